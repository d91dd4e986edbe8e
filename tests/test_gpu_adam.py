"""dsn_adam_step and dsnerf_amd.optim on the device: p, m and v as uint32 words against the numpy restatement of include/dsnerf.h's rule
(tests/adam_restate.py) - every word equal, a NaN for a NaN (IEEE leaves a NaN's payload open) -, the packed image the step leaves
behind against a fresh pack of the new parameters, and the optimizer end to end on the small body beside torch.optim.Adam at the
bar of tests/test_adam_host.py (tests/golden/adam_errors.json x its margin)."""
import copy
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import adam_restate as AR
from helpers import GOLDEN, load

pytestmark = pytest.mark.gpu

BETAS, EPS = (0.9, 0.999), 1e-8
SIZES = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, (1 << 20) + 37]
GUARD = 8          # float32 words of 0xFF around every device array: a store outside a tensor shows


@pytest.fixture(scope="module")
def L():
    import dsnerf_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert (dsnerf_amd._lib.ADAM_TABLE, dsnerf_amd._lib.ADAM_BLOCK) == (AR.TABLE, AR.BLOCK)
    return dsnerf_amd._lib


def same_words(got, want):
    got, want = np.ascontiguousarray(got, np.float32).ravel(), np.ascontiguousarray(want, np.float32).ravel()
    return got.shape == want.shape and bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))


_state = {}


def host_state(n, seed=0, t=1):
    """(p, g, m, v) of n elements, shared by the tests and never written: gradients over seven decades, moments as after a few steps"""
    key = (n, seed, t > 1)
    if key not in _state:
        rng = np.random.RandomState(1000 + 31 * seed + n % 9973)
        p = rng.randn(n).astype(np.float32)
        g = (rng.randn(n) * 10.0 ** rng.uniform(-6, 1, n)).astype(np.float32)
        if t > 1:
            m = (g * rng.uniform(0.5, 1.5, n)).astype(np.float32)
            v = ((g.astype(np.float64) ** 2) * rng.uniform(0.0, 2.0, n)).astype(np.float32)
        else:
            m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
        _state[key] = (p, g, m, v)
    return _state[key]


class Dev:
    """one host array on the device inside a 0xFF-filled buffer, `off` float32 words behind its 16-byte aligned start"""

    def __init__(self, a, off=0):
        a = np.ascontiguousarray(a, np.float32)
        self.n, self.off = a.size, off
        self.buf = torch.empty(a.size + 2 * GUARD, dtype=torch.float32, device="cuda")
        self.buf.view(torch.int32).fill_(-1)
        lo = GUARD + off
        self.t = self.buf[lo:lo + a.size].view(a.shape)
        assert self.t.is_contiguous() and (a.size == 0 or self.t.data_ptr() % 16 == (4 * off) % 16)
        self.t.copy_(torch.from_numpy(a))

    def numpy(self):
        words = self.buf.view(torch.int32).cpu().numpy()
        lo = GUARD + self.off
        assert (words[:lo] == -1).all() and (words[lo + self.n:] == -1).all(), "a store outside the tensor"
        return self.t.cpu().numpy()


def run(L, tensors, lrs, wds, t, offs=(0, 0, 0, 0), betas=BETAS, eps=EPS, packed=None, steps=1):
    """tensors: a list of (p, g, m, v) host arrays (g may be None); one dsn_adam_step call over all of them per step, compared with
    the restatement tensor by tensor; returns the device results [(p, m, v)] as numpy"""
    count = len(tensors)
    lrs = [lrs] * count if np.isscalar(lrs) else list(lrs)
    wds = [wds] * count if np.isscalar(wds) else list(wds)
    dev = [[None if a is None else Dev(a, o) for a, o in zip(row, offs)] for row in tensors]
    want = [[row[0], row[2], row[3]] for row in tensors]
    for k in range(steps):
        L.adam_step([d[0].t for d in dev], [None if d[1] is None else d[1].t for d in dev], [d[2].t for d in dev], [d[3].t for d in dev],
                    lrs, wds, betas, eps, t + k, packed=packed)
        for i, row in enumerate(tensors):
            if row[1] is not None:
                want[i] = list(AR.step32(want[i][0], row[1], want[i][1], want[i][2], AR.scalars(lrs[i], wds[i], betas, eps, t + k)))
    got = []
    for i, d in enumerate(dev):
        res = (d[0].numpy(), d[2].numpy(), d[3].numpy())
        if d[1] is not None:
            assert same_words(d[1].numpy(), tensors[i][1]), "the gradient was written"
        for name, a, b in zip("pmv", res, want[i]):
            assert same_words(a, b), (f"tensor {i} of {count}, {name}': {int((a.ravel().view(np.uint32) != np.asarray(b, np.float32).ravel().view(np.uint32)).sum())} "
                                      f"of {a.size} words differ", t, lrs[i], wds[i])
        got.append(res)
    return got


# ---- the kernel against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_single_tensors_bit_for_bit(L, n):
    """every size around a thread's four elements and a workgroup's 1024, an empty tensor and one of 1025 workgroups; steps 1 (zero
    moments), 2 and 1000, with and without weight decay"""
    for t in (1, 2, 1000):
        for wd in (0.0, 0.01):
            run(L, [host_state(n, 0, t)], 5e-4, wd, t)


def test_all_model_shapes_in_one_call_with_two_groups(L):
    tensors = [tuple(a.reshape(s) for a in host_state(int(np.prod(s)), i, 2)) for i, s in enumerate(AR.SHAPES)]
    lrs = [0.0 if i < 9 else 5e-4 for i in range(33)]             # the frozen / active form of solver/build.py:13-15
    wds = [0.01 if i % 2 else 0.0 for i in range(33)]             # (param groups may differ in decay too)
    got = run(L, tensors, lrs, wds, 3)
    for i in range(9):                                            # lr = 0: p keeps its bits while m and v move
        assert same_words(got[i][0], tensors[i][0])
        assert not same_words(got[i][1], tensors[i][2]) and not same_words(got[i][2], tensors[i][3])


def test_a_hundred_tensors_take_several_tables(L):
    assert 100 > 2 * AR.TABLE
    tensors = [host_state(1 + (37 * i) % 301, i, 2) for i in range(100)]
    tensors[AR.TABLE - 1] = host_state(3 * AR.BLOCK + 5, 7, 2)    # several workgroups at a table's end and at the next one's start
    tensors[AR.TABLE] = host_state(2 * AR.BLOCK, 8, 2)
    run(L, tensors, [1e-4 * (1 + i % 5) for i in range(100)], 0.01, 17)


@pytest.mark.parametrize("offs", [(1, 0, 0, 0), (0, 1, 0, 0), (1, 1, 1, 1), (3, 2, 1, 0)], ids=["p", "g", "all", "mixed"])
def test_views_off_the_16_byte_grid(L, offs):
    """a tensor that starts 4 bytes into a larger buffer: p only, g only, all four (and all at different offsets) - the scalar path of a
    whole segment, beside aligned segments in the same call"""
    tensors = [host_state(n, 3, 2) for n in (5, 1025, 4 * AR.BLOCK + 3)]
    run(L, tensors, 5e-4, 0.01, 2, offs=offs)
    aligned = [Dev(a) for a in host_state(1025, 4, 2)]
    views = [Dev(a, o) for a, o in zip(host_state(1023, 5, 2), offs)]
    L.adam_step([aligned[0].t, views[0].t], [aligned[1].t, views[1].t], [aligned[2].t, views[2].t], [aligned[3].t, views[3].t],
                5e-4, 0.0, BETAS, EPS, 2)
    for d, key in ((aligned, (1025, 4)), (views, (1023, 5))):
        want = AR.step32(*host_state(key[0], key[1], 2), AR.scalars(5e-4, 0.0, BETAS, EPS, 2))
        assert same_words(d[0].numpy(), want[0]) and same_words(d[2].numpy(), want[1]) and same_words(d[3].numpy(), want[2])


def test_a_tensor_without_gradient_is_skipped(L):
    tensors = [host_state(n, 6, 2) for n in (300, 1025, 64, 2050)]
    p, g, m, v = tensors[1]
    tensors[1] = (p, None, m, v)
    got = run(L, tensors, 5e-4, 0.01, 2)
    assert same_words(got[1][0], p) and same_words(got[1][1], m) and same_words(got[1][2], v)
    tensors[3] = (tensors[3][0], None, tensors[3][2], tensors[3][3])      # ... and at the end; then none at all
    run(L, tensors, 5e-4, 0.01, 2)
    run(L, [(p, None, m, v)], 5e-4, 0.0, 2)


def test_edge_values(L):
    """g = 0 with v = 0 (0 / eps = 0: nothing moves), denormal gradients (the square underflows, m stays denormal), huge ones (the
    square overflows: v' = inf, the step 0), infinite and NaN gradients: everything propagates as the rule says, nothing is skipped"""
    n = 1030
    p, g, m, v = (a.copy() for a in host_state(n, 9, 1))
    g[:] = 0.0
    got = run(L, [(p, g, m, v)], 5e-4, 0.0, 1)
    assert same_words(got[0][0], p) and not got[0][1].any() and not got[0][2].any()
    p, g, m, v = (a.copy() for a in host_state(n, 9, 2))
    specials = np.array([1e-45, -1e-45, 1e-40, -3e-39, 1.1754942e-38, 1e30, -1e30, 3.4e38, np.inf, -np.inf, np.nan, 0.0, -0.0], np.float32)
    g[:] = np.resize(specials, n)
    m[::2] = 0.0
    v[::3] = 0.0
    m[5::7] = 1e-42
    for wd in (0.0, 0.01):
        got = run(L, [(p, g, m, v)], 5e-4, wd, 2)
        assert np.isnan(got[0][0]).sum() >= n // len(specials) and np.isinf(got[0][2]).any()
    run(L, [(p, g, m, v)], 5e-4, 0.01, 2, steps=2)                # ... and the NaN / inf moments through a second step


def test_same_call_same_bits_and_consecutive_steps(L):
    tensors = [host_state(n, 10, 2) for n in (1025, 77, 5 * AR.BLOCK + 1)]
    first = run(L, tensors, 5e-4, 0.01, 5)
    again = run(L, tensors, 5e-4, 0.01, 5)
    for a, b in zip(first, again):
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
    run(L, tensors, 5e-4, 0.01, 1, steps=3)                       # three calls with t = 1, 2, 3: three restatement steps
    run(L, [host_state(n, 10, 1) for n in (1025, 77)], 3e-4, 0.0, 1, steps=3)


def test_binding_refuses_what_the_kernel_cannot_take(L):
    p, g, m, v = (Dev(a).t for a in host_state(64, 11, 2))
    with pytest.raises(ValueError):
        L.adam_step([p], [g.double()], [m], [v], 5e-4, 0.0, BETAS, EPS, 1)
    with pytest.raises(ValueError):
        L.adam_step([p], [g], [m[:32]], [v], 5e-4, 0.0, BETAS, EPS, 1)
    with pytest.raises(ValueError):
        L.adam_step([p.reshape(8, 8).t()], [g], [m], [v], 5e-4, 0.0, BETAS, EPS, 1)
    with pytest.raises(ValueError):
        L.adam_step([p], [g], [m], [v.cpu()], 5e-4, 0.0, BETAS, EPS, 1)
    with pytest.raises(ValueError):
        L.adam_step([p], [g], [m], [v], 5e-4, 0.0, BETAS, EPS, 1, packed=L.PackedParams("cuda:0"))
    with pytest.raises(RuntimeError, match="dsn_adam_step"):
        L.adam_step([p], [g], [m], [v], 5e-4, 0.0, BETAS, EPS, 0)
    with pytest.raises(RuntimeError, match="dsn_adam_step"):
        L.adam_step([p], [g], [m], [v], 5e-4, 0.0, (0.9, 1.0), EPS, 1)
    assert same_words(p.cpu().numpy(), host_state(64, 11, 2)[0])


# ---- dsnerf_amd.optim ------------------------------------------------------------------------------------------------------------
def bar_per_tensor():
    """the bar of tests/test_adam_host.py's comparison with torch: per tensor, its margin x the largest recorded distance of
    torch-float32 from float64 over the recorded cases"""
    with open(os.path.join(GOLDEN, "adam_errors.json")) as f:
        rec = json.load(f)
    return {k: rec["margin"] * max(rec["cases"][c][k]["torch_float32"] for c in rec["cases"]) for k in rec["cases"]["plain"]}


def model_net(seed=0):
    import dsnerf_amd
    from cases import make_cfg, state
    net = dsnerf_amd.DualSpaceNeRF(make_cfg(16))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state().items()})
    net.cuda()
    rng = np.random.RandomState(40 + seed)
    grads = {k: torch.from_numpy((rng.randn(*p.shape) * 10.0 ** rng.uniform(-5, 0, p.shape)).astype(np.float32)).cuda()
             for k, p in net.named_parameters()}
    return net, grads


def set_grads(net, grads):
    for k, p in net.named_parameters():
        p.grad = grads[k].clone()


def fresh_image(L, net):
    """the image a pack of the net's parameters, as they are now, writes into a 0xFF-filled buffer"""
    ref = L.PackedParams(next(net.parameters()).device)
    ref.buf.fill_(255)
    ref.update(dict(net.named_parameters()), force=True)
    return ref.buf


def test_step_bits_and_the_packed_image(L):
    """optim.Adam(net.parameters(), net=net): three steps give three restatement steps on all 33 tensors (step counts 1, 2, 3 on the
    host, float32), every version counter advances, and the image behind each step is a fresh pack's, byte for byte, with the
    bookkeeping of a re-pack: generation + 1, calibrations dropped, and nothing left for net.packed() to do"""
    import dsnerf_amd
    net, grads = model_net()
    named = dict(net.named_parameters())
    want = {k: [p.detach().cpu().numpy(), np.zeros(p.shape, np.float32), np.zeros(p.shape, np.float32)] for k, p in named.items()}
    opt = dsnerf_amd.optim.Adam(net.parameters(), lr=5e-4, weight_decay=0.01, net=net)
    packed = net.packed()
    packed.screen, packed.early_stop = {"usable": True}, {"usable": True}
    for t in (1, 2, 3):
        set_grads(net, grads)
        gen = packed.generation
        versions = {k: p._version for k, p in named.items()}
        packed.buf.fill_(255)
        opt.step()
        for k, p in named.items():
            want[k] = list(AR.step32(want[k][0], grads[k].cpu().numpy(), want[k][1], want[k][2], AR.scalars(5e-4, 0.01, BETAS, EPS, t)))
            st = opt.state[p]
            assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
            assert st["step"].dtype == torch.float32 and st["step"].dim() == 0 and not st["step"].is_cuda and float(st["step"]) == t
            for name, a, b in (("p", p, want[k][0]), ("m", st["exp_avg"], want[k][1]), ("v", st["exp_avg_sq"], want[k][2])):
                assert same_words(a.detach().cpu().numpy(), b), (k, name, t)
            assert p._version > versions[k], k
        assert net._packed is packed and packed.generation == gen + 1 and packed.screen is None and packed.early_stop is None
        assert packed.colour_scale == 1.0
        assert torch.equal(packed.buf, fresh_image(L, net)), f"step {t}: the image is not a pack of the new parameters"
        seen = packed._versions
        assert net.packed() is packed and packed.generation == gen + 1 and packed._versions == seen          # nothing to re-pack
        assert seen == tuple((named[k].data_ptr(), named[k]._version) for k in L.PARAM_ORDER)
    # a parameter without a gradient: skipped, its step count stays, the image is still rebuilt from all 33
    set_grads(net, grads)
    lone = named["nerf.stage1.2.bias"]
    lone.grad = None
    before = lone.detach().clone()
    gen = packed.generation
    opt.step()
    assert torch.equal(lone.detach(), before) and float(opt.state[lone]["step"]) == 3.0
    assert float(opt.state[named["nerf.stage1.2.weight"]]["step"]) == 4.0
    # (its step count now differs from the others': the next step's tensors share one count again, the lone one is without gradient)
    assert packed.generation == gen + 1 and torch.equal(packed.buf, fresh_image(L, net))


def test_without_net_the_next_packed_call_repacks(L):
    import dsnerf_amd
    net, grads = model_net(1)
    packed = net.packed()
    gen = packed.generation
    assert net.packed().generation == gen
    opt = dsnerf_amd.optim.Adam(net.parameters(), lr=5e-4)
    set_grads(net, grads)
    opt.step()
    assert packed.generation == gen                                # the step did not touch the image ...
    assert net.packed() is packed and packed.generation == gen + 1  # ... the version counters made packed() rebuild it
    assert torch.equal(packed.buf, L.PackedParams(packed.device).update(dict(net.named_parameters()), force=True).buf)
    # net= with only some of the parameters: not honoured, same behaviour
    some = [p for k, p in net.named_parameters() if k.startswith("nerf.")]
    opt = dsnerf_amd.optim.Adam(some, lr=5e-4, net=net)
    set_grads(net, grads)
    gen = packed.generation
    opt.step()
    assert packed.generation == gen and net.packed().generation == gen + 1


def test_constructor_groups_and_make_optimizer(L):
    import dsnerf_amd
    net, grads = model_net(2)
    params = list(net.parameters())
    for kw in ("amsgrad", "maximize", "capturable", "differentiable", "fused", "foreach"):
        with pytest.raises(ValueError, match=kw):
            dsnerf_amd.optim.Adam(params, **{kw: True})
    with pytest.raises(ValueError):
        dsnerf_amd.optim.Adam([torch.nn.Parameter(torch.zeros(4, device="cuda", dtype=torch.float64))])
    with pytest.raises(ValueError):
        dsnerf_amd.optim.Adam([torch.nn.Parameter(torch.zeros(4, 4, device="cuda").t())])
    with pytest.raises(ValueError):
        dsnerf_amd.optim.Adam([torch.nn.Parameter(torch.zeros(4))])
    cfg = SimpleNamespace(SOLVER=SimpleNamespace(WEIGHT_DECAY=0.01, BASE_LR=5e-4, OPTIMIZER_NAME="Adam"))
    one = dsnerf_amd.optim.make_optimizer(cfg, net)
    ref = torch.optim.Adam(params=net.parameters(), lr=5e-4, betas=(0.9, 0.999), weight_decay=0.01)
    assert isinstance(one, torch.optim.Optimizer) and len(one.param_groups) == 1 and one._net() is net and one._net_params is not None
    assert set(one.param_groups[0]) == set(ref.param_groups[0])
    assert {k: v for k, v in one.param_groups[0].items() if k != "params"} == {k: v for k, v in ref.param_groups[0].items() if k != "params"}
    frozen = [p for k, p in net.named_parameters() if k.startswith("pose_mlp.")]
    active = [p for k, p in net.named_parameters() if not k.startswith("pose_mlp.")]
    two = dsnerf_amd.optim.make_optimizer(cfg, net, active_list=active, frozen_list=frozen)
    assert [g["lr"] for g in two.param_groups] == [0.0, 5e-4] and [len(g["params"]) for g in two.param_groups] == [6, 27]
    # the schedule of solver/lr_scheduler.py:58-71 drives it unchanged: LambdaLR writes group["lr"], step() reads it on every call
    factor = AR.schedule(4.0, 6.0, 9.0, 0.1)
    sched = torch.optim.lr_scheduler.LambdaLR(optimizer=two, lr_lambda=[factor] * len(two.param_groups))
    named = dict(net.named_parameters())
    initial = {k: p.detach().cpu().numpy().copy() for k, p in named.items()}
    want = {k: [initial[k], np.zeros(p.shape, np.float32), np.zeros(p.shape, np.float32)] for k, p in named.items()}
    packed = net.packed()
    for k in range(7):
        set_grads(net, grads)
        two.step()
        sched.step()
        for name, p in named.items():
            lr = 0.0 if name.startswith("pose_mlp.") else 5e-4 * factor(k)
            want[name] = list(AR.step32(want[name][0], grads[name].cpu().numpy(), want[name][1], want[name][2], AR.scalars(lr, 0.01, BETAS, EPS, k + 1)))
    for name, p in named.items():
        assert same_words(p.detach().cpu().numpy(), want[name][0]), name
        if name.startswith("pose_mlp."):
            assert same_words(p.detach().cpu().numpy(), initial[name])          # the frozen group did not move
    assert torch.equal(packed.buf, L.PackedParams(packed.device).update(named, force=True).buf)


def test_parameters_beside_the_net_are_updated_too(L):
    """an optimizer that holds more than the net's 33 tensors - a latent table in the net's group, a second group of its own, one added
    later - with net=: every tensor follows the restatement bit for bit, the image is still rebuilt by the step, and the next
    net.packed() launches nothing"""
    import dsnerf_amd
    net, grads = model_net(4)
    rng = np.random.RandomState(9)
    extra = {k: torch.nn.Parameter(torch.from_numpy(rng.randn(*shape).astype(np.float32)).cuda())
             for k, shape in (("latent", (37, 5)), ("own_group", (1025,)), ("added_later", (3,)))}
    egrads = {k: torch.from_numpy((rng.randn(*p.shape) * 1e-2).astype(np.float32)).cuda() for k, p in extra.items()}
    lrs = {"latent": 5e-4, "own_group": 2e-3, "added_later": 1e-4}
    opt = dsnerf_amd.optim.Adam([{"params": list(net.parameters()) + [extra["latent"]]}, {"params": [extra["own_group"]], "lr": 2e-3}],
                                lr=5e-4, weight_decay=0.01, net=net)
    assert opt._net_params is not None
    every = dict(net.named_parameters(), latent=extra["latent"], own_group=extra["own_group"])
    every_g = dict(grads, **egrads)
    want = {k: [p.detach().cpu().numpy(), np.zeros(p.shape, np.float32), np.zeros(p.shape, np.float32)] for k, p in every.items()}
    packed = net.packed()
    for t in (1, 2, 3):
        if t == 3:                                                # its step count starts at 1 while the others' is 3: a call of its own
            opt.add_param_group({"params": [extra["added_later"]], "lr": 1e-4})
            assert opt._net_params is not None
            every["added_later"] = extra["added_later"]
            want["added_later"] = [extra["added_later"].detach().cpu().numpy(), np.zeros(3, np.float32), np.zeros(3, np.float32)]
        for k, p in every.items():
            p.grad = every_g[k].clone()
        gen = packed.generation
        versions = {k: p._version for k, p in every.items()}
        opt.step()
        for k, p in every.items():
            tk = 1 if k == "added_later" else t
            want[k] = list(AR.step32(want[k][0], every_g[k].cpu().numpy(), want[k][1], want[k][2], AR.scalars(lrs.get(k, 5e-4), 0.01, BETAS, EPS, tk)))
            st = opt.state[p]
            assert float(st["step"]) == tk and p._version > versions[k], k
            for name, a, b in (("p", p, want[k][0]), ("m", st["exp_avg"], want[k][1]), ("v", st["exp_avg_sq"], want[k][2])):
                assert same_words(a.detach().cpu().numpy(), b), (k, name, t)
        assert packed.generation == gen + 1 and net.packed() is packed and packed.generation == gen + 1
        assert torch.equal(packed.buf, L.PackedParams(packed.device).update(dict(net.named_parameters()), force=True).buf)
    # a copy of the optimizer carries no binding (and not the model): it updates its own parameters and leaves images alone
    clone = copy.deepcopy(opt)
    assert clone._net is None and clone._net_params is None and len(clone.param_groups) == 3
    for g in clone.param_groups:
        for q in g["params"]:
            q.grad = torch.zeros_like(q)
    clone.step()
    assert packed.generation == gen + 1


def test_a_refused_gradient_leaves_everything_as_it_was(L):
    """a sparse gradient and a float64 one raise ValueError from step() before any step count has advanced or any tensor has been
    touched - also for the parameter in front of the offending one"""
    import dsnerf_amd
    a = torch.nn.Parameter(torch.from_numpy(host_state(300, 12, 2)[0]).cuda())
    b = torch.nn.Parameter(torch.from_numpy(host_state(64, 12, 2)[0]).cuda())
    opt = dsnerf_amd.optim.Adam([a, b], lr=5e-4)
    a.grad, b.grad = torch.ones_like(a), torch.ones_like(b)
    opt.step()
    kept = [a.detach().clone(), b.detach().clone(), opt.state[a]["exp_avg"].clone()]
    versions = (a._version, b._version)
    sparse = torch.sparse_coo_tensor(torch.tensor([[1, 5]], device="cuda"), torch.ones(2, device="cuda"), (64,))
    b.grad_dtype = None                                            # (torch itself refuses a float64 .grad on a float32 tensor unless told so)
    for bad, what in ((sparse, "sparse"), (torch.ones(64, device="cuda", dtype=torch.float64), "float32")):
        b.grad = None
        b.grad = bad
        with pytest.raises(ValueError, match=what):
            opt.step()
        assert float(opt.state[a]["step"]) == 1.0 and float(opt.state[b]["step"]) == 1.0
        assert torch.equal(a.detach(), kept[0]) and torch.equal(b.detach(), kept[1]) and torch.equal(opt.state[a]["exp_avg"], kept[2])
        assert (a._version, b._version) == versions
    b.grad = None
    b.grad = torch.ones_like(b)
    opt.step()                                                     # ... and the optimizer goes on from there
    assert float(opt.state[a]["step"]) == 2.0 and float(opt.state[b]["step"]) == 2.0


def test_state_dict_goes_both_ways(L):
    """a torch.optim.Adam that ran three steps on the GPU hands its state_dict to optim.Adam; one step of each from there agrees at
    the bar of the host test; and optim.Adam's own state_dict loads into a torch.optim.Adam, equal keys and dtypes"""
    import dsnerf_amd
    bar = bar_per_tensor()
    net, grads = model_net(3)
    other, _ = model_net(3)
    topt = torch.optim.Adam(other.parameters(), lr=5e-4, weight_decay=0.01)
    for _ in range(3):
        set_grads(other, grads)
        topt.step()
    net.load_state_dict(other.state_dict())
    opt = dsnerf_amd.optim.Adam(net.parameters(), lr=1e-3, net=net)
    sd = topt.state_dict()
    opt.load_state_dict(copy.deepcopy(sd))
    assert opt.param_groups[0]["lr"] == 5e-4 and opt.param_groups[0]["weight_decay"] == 0.01
    mine = opt.state_dict()
    assert set(mine) == set(sd) and [set(g) for g in mine["param_groups"]] == [set(g) for g in sd["param_groups"]]
    for j in sd["state"]:
        assert set(mine["state"][j]) == set(sd["state"][j])
        for k in sd["state"][j]:
            a, b = mine["state"][j][k], sd["state"][j][k]
            assert a.dtype == b.dtype and a.device == b.device and torch.equal(a, b), (j, k)
    set_grads(other, grads)
    set_grads(net, grads)
    topt.step()
    opt.step()
    from cases import rel
    for (k, p), q in zip(net.named_parameters(), other.parameters()):
        d = rel(p.detach().cpu().numpy(), q.detach().cpu().numpy())
        print(f"one step after load_state_dict: {k} relative L2 {d:.3e} (bar {bar[k]:.3e})")
        assert d <= bar[k], (k, d, bar[k])
        assert float(opt.state[p]["step"]) == 4.0
    assert torch.equal(net._packed.buf, L.PackedParams(net._packed.device).update(dict(net.named_parameters()), force=True).buf)
    # ... and back: torch continues from optim.Adam's state
    back = torch.optim.Adam(other.parameters(), lr=1e-3)
    back.load_state_dict(copy.deepcopy(opt.state_dict()))
    set_grads(other, grads)
    back.step()
    assert all(float(back.state[q]["step"]) == 5.0 and back.state[q]["step"].dtype == torch.float32 for q in other.parameters())
    # a group option it does not implement is refused when it arrives through a state_dict too
    bad = copy.deepcopy(sd)
    bad["param_groups"][0]["amsgrad"] = True
    with pytest.raises(ValueError, match="amsgrad"):
        opt.load_state_dict(bad)


def _cfg_loss():
    return SimpleNamespace(MODEL=SimpleNamespace(LOSS="L2", LOSSwMask=True))


def test_training_end_to_end_beside_torch_adam(L):
    """trainer.py:66-81 in miniature on the small body: sample_batch -> render -> make_loss -> backward -> step with optim.Adam (net=)
    and with torch.optim.Adam from the same start and the same draws.  The losses fall in both runs, the parameters of the two runs
    agree per tensor at the host test's bar, render_view gives the same bits before training and after the initial state_dict is
    restored, and a step() between a render and its backward still makes that backward raise.
    The two live runs are compared after STEPS = 3 steps: the first (zero moments), the second (the moments in use) and one more.  The
    training backward sums its weight gradients with floating-point atomics, so two runs of ONE optimizer already differ (measured,
    torch.optim.Adam against itself: gradients 7e-8 relative L2 at step 1, parameters 2e-8 at step 3 and 4e-8 at step 6; optim.Adam
    against torch.optim.Adam 5e-8 and 7e-8), and over more steps that noise can tip a discrete decision of the renderer (seen at step
    6: 8e-4 in a gradient, 1.7e-6 in the parameters, between torch's foreach and single-tensor forms as well).  What separates the two
    optimizers alone is pinned over six steps without that noise: torch.optim.Adam fed the gradients optim.Adam's run saw, same bar."""
    import dsnerf_amd
    import train_rays_restate as TR
    from cases import make_batch, make_renderer, rel
    bar = bar_per_tensor()
    g = load("small_eval")
    r = make_renderer(g, "small_eval")
    gv = load("small_view")
    Hv, Wv = int(gv["H"]), int(gv["W"])

    def view():
        r.eval()
        b = make_batch(gv)
        b["img"] = torch.zeros(1, Hv, Wv, 3, dtype=torch.float64)
        b["mask_at_box"] = torch.from_numpy(gv["mask_at_box"])[None]
        out = {k: v.clone() for k, v in r.render_view(b).items() if torch.is_tensor(v)}
        r.train()
        return out

    start = copy.deepcopy(r.net.state_dict())
    before = view()
    xyz = g["xyz"]
    lo, hi = xyz.min(0) - 0.05, xyz.max(0) + 0.05
    H, W = 37, 53
    f = 0.9 * W
    K = np.array([[f, 0.0, W / 2 - 0.5], [0.0, f, H / 2 - 0.5], [0.0, 0.0, 1.0]])
    Rm, T = np.eye(3), np.array([0.0, 0.0, 3.0]) - (lo + hi) / 2
    bounds = np.stack([lo, hi]).astype(np.float64)
    rng = np.random.RandomState(2)
    img = torch.from_numpy(rng.rand(H, W, 3)).cuda()
    mask = torch.from_numpy(TR.bound_mask(K, Rm, T, bounds, H, W) * (rng.rand(H, W) < 0.5)).cuda()
    batch = r.sample_batch(img, K, Rm, T, bounds, mask, 64, 77, occupancy_from=mask)
    extra = make_batch(g)
    batch.update(xyz=extra["xyz"], poses=extra["poses"], frame=extra["frame"], Th=extra["Th"])
    cfg = SimpleNamespace(SOLVER=SimpleNamespace(WEIGHT_DECAY=0.0, BASE_LR=5e-4, OPTIMIZER_NAME="Adam"))
    loss_fn = dsnerf_amd.loss.make_loss(_cfg_loss())

    STEPS = 3

    def train(opt, steps, replay=None):
        """returns the losses, the parameters after STEPS steps and at the end, and the gradients of every step"""
        losses, seen, at = [], [], None
        for k in range(steps):
            torch.manual_seed(100)                                 # (the same jitter and noise on every step: the loss is a function of the parameters)
            opt.zero_grad()
            if replay is None:
                loss1 = loss_fn(r.render(batch)["coarse"], batch)
                loss = 0
                for key in loss1:
                    loss += loss1[key]
                loss.backward()
                losses.append(loss.detach())
                seen.append([p.grad.detach().clone() for p in r.net.parameters()])
            else:
                for p, gr in zip(r.net.parameters(), replay[k]):
                    p.grad = gr.clone()
            opt.step()
            if k + 1 in (STEPS, steps):
                now = {k_: p.detach().cpu().numpy().copy() for k_, p in r.net.named_parameters()}
                at = at or now
        return [float(v) for v in losses], at, now, seen

    def torch_adam():
        return torch.optim.Adam(params=r.net.parameters(), lr=5e-4, betas=(0.9, 0.999), weight_decay=0.0)

    def within_bar(what, a, b):
        worst = {k: rel(a[k], b[k]) for k in a}
        for k in a:
            print(f"{what}: {k} relative L2 {worst[k]:.3e} (bar {bar[k]:.3e})")
        for k in a:
            assert worst[k] <= bar[k], (what, k, worst[k], bar[k])

    opt = dsnerf_amd.optim.make_optimizer(cfg, r.net)
    gen = r.net.packed().generation
    mine_losses, mine3, mine6, seen = train(opt, 6)
    assert r.net._packed.generation == gen + 6                    # one rebuild per step, none by the renders
    # the autograd guard: the parameters a render saved are stale after a step
    torch.manual_seed(1)
    loss1 = loss_fn(r.render(batch)["coarse"], batch)
    opt.step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (loss1["loss_rgb"] + loss1["loss_mask"]).backward()
    r.net.load_state_dict(start)
    after = view()
    for k in before:
        assert torch.equal(before[k].contiguous().view(torch.uint8), after[k].contiguous().view(torch.uint8)), k
    theirs_losses, theirs3, _, _ = train(torch_adam(), STEPS)
    print("losses, optim.Adam:", mine_losses, "torch.optim.Adam:", theirs_losses)
    for losses in (mine_losses, theirs_losses):
        assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    within_bar(f"{STEPS} steps, optim.Adam against torch.optim.Adam", mine3, theirs3)
    r.net.load_state_dict(start)
    _, _, replayed6, _ = train(torch_adam(), 6, replay=seen)
    within_bar("6 steps, torch.optim.Adam on the gradients optim.Adam saw", mine6, replayed6)
    assert r.range_overflow_count() == 0
