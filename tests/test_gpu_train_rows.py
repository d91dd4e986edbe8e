"""The training backward at CHOSEN row counts (tests/train_rows_cases.py): dsn_module_grad and dsn_render_rays_grad on batches whose
two row lists hold exactly the counts at which the weight-gradient products, the field passes and the small GEMMs change their code
path - short prologues (a second workgroup with 16 / 32 / 48 rows), register-load tails, empty shares, one- and four-address
staging, counts of 0 and 1, all-zero cotangents - against the float64 oracle, per tensor, at a bar the oracle sets itself (a tenth
of what ONE row moves the gradient; never above the suite's ceiling of 5e-3).

Every case runs on a workspace whose previous batches had the same size and filled both lists (history()): the slots behind the
case's counts then hold valid row numbers, and a kernel that reads past a count gives a wrong gradient - which the comparison
catches - and no fault.

The largest errors are those of the all-transparent pool at the converged parameters with few live rows (6.9e-4 at F = 17 on
lighting_mlp.lights_encoding.4.bias, falling to 3e-5 at F = 257; the float32 oracle differs from the float64 one by 1e-4 there):
single samples far outside the body, the same at F = 15, 16 and 17.  Why they are that noisy has not been measured.

Each case prints one `train_rows:` line: the worst error / bar over the 33 tensors and the tensor it belongs to
(profiles/train_rows_errors.txt is that output)."""
import numpy as np
import pytest
import torch

import train_rows_cases as C
from cases import make_batch, make_renderer

pytestmark = pytest.mark.gpu

CASES = C.all_cases()
HISTORY = [c for c in CASES if (c[0].startswith("A2-") and int(c[0].rsplit("B", 1)[1]) in C.HISTORY_COUNTS)
           or (c[0].startswith("B-pure-") and int(c[0].rsplit("F", 1)[1]) in C.HISTORY_COUNTS)]


class Device:
    """one parameter set on the device: scene with the fixture's frame set, parameters, their packed image, ONE gradient workspace
    (renderer: one that exists already, its scene's frame set)"""

    def __init__(self, name, renderer=None):
        from dsnerf_amd import _lib
        from cases import state
        self.lib, self.name = _lib, name
        self.g = C.fixture(name)
        self.r = renderer
        if renderer is None:
            self.r = make_renderer(self.g, name)
            self.r._set_frame(make_batch(self.g))
        self.dev = self.r.device
        self.params = {k: torch.from_numpy(v).to(self.dev) for k, v in state(name).items()}
        self.packed = _lib.PackedParams(self.dev).update(self.params)
        self.poses = self.T(self.g["poses"])
        self.ws = _lib.GradWorkspace(self.dev)

    def T(self, a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def run(self, c, ws=None):
        """-> ({tensor: float64 array}, (forward rows, backward rows), samples that left the fp16 range)"""
        L, ws = self.lib, ws or self.ws
        if c.mode == "module":
            grads = L.module_grad(self.r.scene, self.params, self.poses, int(self.g["frame"]), False, self.T(c.x_w), self.T(c.x_c),
                                  self.T(c.view), self.T(c.gc), self.T(c.gs), ws=ws, packed=self.packed)
            shape = (c.N, 1)
        else:
            grads = L.render_rays_grad(self.r.scene, self.params, self.poses, int(self.g["frame"]), False, self.T(c.o), self.T(c.d), self.T(c.z),
                                       self.T(c.noise), self.T(c.cot["color"]), self.T(c.cot["disp_map"]), self.T(c.cot["acc_map"]),
                                       self.T(c.cot["depth_map"]), self.T(c.cot["weights"]), ws=ws, packed=self.packed)
            shape = (c.R, c.S)
        got = {k: v.double().cpu().numpy() for k, v in zip(L.PARAM_ORDER, grads)}
        return got, L.grad_row_counts(ws, *shape), L.grad_range_overflow(ws, *shape)

    def history(self, c, ws=None):
        """the batches in front of a case, same N: every row live and every cotangent non-zero (fills list1, and list2 wherever no
        cotangent underflows), then - ray mode - N explicit points with a cotangent each, which fills list2 whatever the rays do"""
        ws = ws or self.ws
        _, rows, _ = self.run(C.all_live(c), ws)
        if c.mode == "rays":
            assert rows[0] == c.N, rows
            _, rows, _ = self.run(C.module_fill(c.name, c.N), ws)
        assert rows[1] == c.N, rows


_DEVICES = {}


def device(name):
    if name not in _DEVICES:
        _DEVICES[name] = Device(name)
    return _DEVICES[name]


def judge(c, got, full=None):
    """33 finite tensors; a tensor the float64 oracle leaves exactly zero is exactly zero; every other one within the case's bar and
    the ceiling.  Prints the case's line"""
    full = C.reference(c) if full is None else full         # (the case's own float64 gradient, kept by its builder)
    assert len(got) == 33 and all(np.isfinite(v).all() for v in got.values()), c.label
    bar, med = C.bar(c, full)
    err, nonzero = C.errors(got, full)
    lim = min(bar, C.CEILING)
    if err:
        k = max(err, key=err.get)
        print(f"train_rows: {c.label}: worst error / bar {err[k] / lim:.3f} ({err[k]:.2e} / {lim:.2e}, median delta {med:.2e}) {k}")
    else:
        print(f"train_rows: {c.label}: no gradient, 33 tensors exactly zero: {not nonzero}")
    assert not nonzero, (c.label, nonzero)
    for k, e in err.items():
        assert e <= lim, (c.label, k, e, lim)
    return full


def check_counts(cid, c, rows):
    if c.mode == "module":
        assert rows[1] == c.backward, (cid, rows, c.backward)              # (module mode has no forward list)
        return
    assert rows[0] == c.forward, (cid, rows, c.forward)
    if cid.startswith("B-pure-") or cid.startswith("C-F0") or cid.startswith("C-B0"):
        assert rows[1] == c.backward, (cid, rows, c.backward)
    elif cid.startswith("B-mixed-"):
        assert c.forward - 128 <= rows[1] <= c.forward, (cid, rows)
    else:                                                                   # zero-cotangent rays, tiny batches
        assert rows[1] <= c.live_with_cotangent, (cid, rows, c.live_with_cotangent)


@pytest.mark.parametrize("cid,family,build", CASES, ids=[c[0] for c in CASES])
def test_chosen_row_counts_match_the_float64_oracle(cid, family, build):
    c = build()
    D = device(c.name)
    D.history(c)
    got, rows, overflow = D.run(c)
    assert overflow == 0, cid
    check_counts(cid, c, rows)
    judge(c, got)


@pytest.mark.parametrize("name", C.PARAM_SETS)
@pytest.mark.parametrize("noise", ["none", "dead"])
def test_forward_without_a_live_row_writes_exact_zeros(name, noise):
    """F = 0 through the training forward (dsn_render_rays_train) on the 64 all-transparent rays, with noise = None and with a noise
    array that is <= 0 everywhere, behind the all-live history: list1 is empty, colour, acc and weights are exactly zero"""
    D = device(name)
    b = C.forward_f0_batch(name)
    L = D.lib
    D.history(C.pure_case(name, 0))
    out = L.render_rays(D.r.scene, D.packed, L.RenderWorkspace(D.dev), D.T(b.o), D.T(b.d), D.T(b.near), D.T(b.far), b.S,
                        torch.linspace(0.0, 1.0, steps=b.S).to(D.dev), None, D.T(b.dead_noise) if noise == "dead" else None,
                        skip_transparent=False, train_cache=D.ws)
    torch.cuda.synchronize()
    assert np.array_equal(out["z_vals"].cpu().numpy(), b.z)                  # the samples whose flags the batch was built on
    assert L.grad_row_counts(D.ws, b.R, b.S)[0] == 0
    for k in ("color", "acc_map", "weights"):
        assert torch.isfinite(out[k]).all() and not bool(out[k].any()), k   # exactly zero


@pytest.mark.parametrize("cid,family,build", HISTORY, ids=[c[0] for c in HISTORY])
def test_stale_list_slots_do_not_reach_a_gradient(cid, family, build):
    """the same case behind two histories - every row live / ONE row live - on workspaces of their own: the slots behind the counts
    differ, the gradients must not.  The trunk's weight gradients (`stage`) come from the two-stage fixed-order reduction: bit for
    bit; the others (atomics) to 2e-6, as test_paired_weight_gradient_launches_match_the_single_ones asks"""
    c = build()
    D = device(c.name)
    one = C.a2_case(c.name, 1, "prefix") if c.mode == "module" else C.pure_case(c.name, 1)
    wa, wb = D.lib.GradWorkspace(D.dev), D.lib.GradWorkspace(D.dev)
    D.history(c, wa)
    a, rows_a, _ = D.run(c, wa)
    D.history(c, wb)                                        # (so that no slot of this workspace is uninitialised memory)
    _, rows_1, _ = D.run(one, wb)
    assert rows_1[1] == 1 and (c.mode == "module" or rows_1[0] == 1), rows_1
    b, rows_b, _ = D.run(c, wb)
    assert rows_a == rows_b or c.mode == "module" and rows_a[1] == rows_b[1]
    for k in a:
        if "stage" in k:
            assert np.array_equal(a[k], b[k]), (cid, k, C.rel(a[k], b[k]))
        else:
            assert C.rel(a[k], b[k]) <= 2e-6 or not np.any(b[k]) and not np.any(a[k]), (cid, k, C.rel(a[k], b[k]))
    judge(c, b)


@pytest.mark.parametrize("name", C.PARAM_SETS)
@pytest.mark.parametrize("F", [C.RENDERER_F, 0])
def test_chosen_row_counts_through_the_renderer(name, F):
    """Renderer.render(...)["coarse"] in train mode + loss.backward(): the cached forward (dsn_render_rays_train, k_light16 / k_normal
    on list1) at a chosen count.  The renderer draws its own noise from the seeded generator - N(0,1) per sample - so the batch is
    the 10 pure-pool rays whose draw at the case's seed leaves exactly 80 of 160 samples live; F = 0: raw_noise_std = 0.  The noise
    is read back from the render's autograd node, z_vals from its output: the oracle and the expected count come from those"""
    from dsnerf_amd import _lib
    c0 = C.renderer_case(name, F)
    g = dict(C.fixture(name))
    g["S"] = np.int64(C.S)
    for k in ("ray_o", "ray_d", "near", "far"):
        g[k] = np.ascontiguousarray(g[k][c0.rays])
    r = make_renderer(g, name)
    r.cfg.MODEL.raw_noise_std = 1.0 if F else 0.0
    r.train()
    r._set_frame(make_batch(g))
    r._grad_ws = _lib.GradWorkspace(r.device)                # the renderer's own workspace, with the history of every other case
    Device(name, renderer=r).history(c0, r._grad_ws)
    torch.manual_seed(c0.seed)
    out = r.render(make_batch(g))["coarse"]
    # what the renderer drew and sampled: the noise it handed to its forward (kept by the autograd node), the z_vals it returned
    drawn = out["color"].grad_fn.call[2]
    z = out["z_vals"].detach().cpu().numpy()
    noise = None if drawn is None else drawn.detach().cpu().numpy()
    assert (noise is None) == (F == 0)
    same = np.array_equal(z, c0.z) and (noise is None or np.array_equal(noise, c0.noise))
    c = c0 if same else C.renderer_case(name, F, z=z, noise=noise)
    assert c.forward == F, (c.forward, F)
    if F == 0:
        for k in ("color", "acc_map", "weights"):
            assert not bool(out[k].any()), k                 # exactly zero
    loss = sum((torch.from_numpy(c.cot[k]).to(r.device) * out[k]).sum() for k in C.OUT_KEYS)
    r.net.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    rows = _lib.grad_row_counts(r._grad_ws, c.R, c.S)
    assert rows[0] == F and rows[1] <= F and (rows[1] == c.backward), (rows, F, c.backward)
    assert r.range_overflow_count() == 0
    got = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().double().cpu().numpy() for k, p in r.net.named_parameters()}
    judge(c, got)
