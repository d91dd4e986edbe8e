"""The training step's draws on the device (dsn_train_draws; _lib.train_draws, Renderer.draws = "device"): the kernel against the
numpy restatement of include/dsnerf.h's rule (tests/draws_restate.py) - the jitter word for word, the noise within one float32 ulp
with at most 0.1 % of a call's values differing at all (the device's float64 log / cos / sin against numpy's: of the order of 1e-8 of
the values cross a float32 rounding boundary; a wrong rule differs nearly everywhere) - on 0xFF-filled buffers over the whole grid of
shapes, and the renderer's use of it: nothing but the source of the draws changes."""
import numpy as np
import pytest
import torch

import draws_restate as DR
from helpers import load

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RS = (0, 1, 63, 64, 65, 257, 8192)
SS = (1, 3, 4, 5, 63, 64, 65, 128)
SEED = (0x9e3779b9 << 32) | 0x7f4a7c15          # a non-zero high word
DIFFER_CAP = 1e-3          # share of a call's noise values that may differ from the restatement at all (a condition, not a measurement)
GUARD = 8                  # floats of 0xFF kept in front of and behind every output


def L():
    import dsnerf_amd
    return dsnerf_amd._lib


def filled(R, S, offset=0):
    """a 0xFF-filled buffer and its [R, S] view `offset` floats behind a 256-byte aligned address + GUARD floats"""
    assert GUARD % 4 == 0
    buf = torch.empty(R * S + 2 * GUARD + 4, dtype=torch.float32, device=DEV)
    buf.view(torch.int32).fill_(-1)
    assert buf.data_ptr() % 16 == 0
    view = buf[GUARD + offset:GUARD + offset + R * S].view(R, S)
    assert R * S == 0 or view.data_ptr() % 16 == (4 * offset) % 16
    return buf, view


def guards_intact(buf, R, S, offset=0):
    w = buf.view(torch.int32)
    return bool((w[:GUARD + offset] == -1).all()) and bool((w[GUARD + offset + R * S:] == -1).all())


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def check_jitter(got, want, what):
    assert np.array_equal(bits(got), want.view(np.uint32)), what


def check_noise(got, want, what):
    g = got.detach().cpu().numpy()
    assert np.all(np.isfinite(g)), what
    d = DR.ulp_distance(g, want)
    differ = int((bits(got) != want.view(np.uint32)).sum())
    assert d.size == 0 or int(d.max()) <= 1, (what, int(d.max()), differ)
    assert differ <= DIFFER_CAP * g.size, (what, differ, g.size)
    return differ


def draw(R, S, seed, step, offset=0, want=(True, True), **kw):
    bufs = [filled(R, S, offset) if w else (None, None) for w in want]
    j, n = L().train_draws(R, S, seed, step, want_jitter=want[0], want_noise=want[1], out=(bufs[0][1], bufs[1][1]), **kw)
    torch.cuda.synchronize()
    for b, _ in bufs:
        assert b is None or guards_intact(b, R, S, offset), (R, S, offset)
    assert (j is None) == (not want[0]) and (n is None) == (not want[1])
    return j, n


# ---- 1. the kernel against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", RS)
def test_bits_against_the_restatement_over_the_grid(R):
    """every S of the grid at this R, each with its own step: aligned outputs (16-byte stores where S % 4 == 0) and outputs 4 bytes off
    the 16-byte grid (scalar stores) hold the same values, nothing is written outside [R, S]"""
    differ = total = 0
    for i, S in enumerate(SS):
        step = 11 * i + R
        want_j, want_n = DR.draws(R, S, SEED, step)
        for offset in (0, 1):
            j, n = draw(R, S, SEED, step, offset)
            assert j.shape == n.shape == (R, S)
            check_jitter(j, want_j, (R, S, offset))
            differ += check_noise(n, want_n, (R, S, offset))
            total += R * S
    print(f"R {R}: {differ} of {total} noise values differ from the restatement (by one ulp)")


def test_fresh_outputs_and_the_empty_call():
    j, n = L().train_draws(65, 7, SEED, 2, device=DEV)
    want_j, want_n = DR.draws(65, 7, SEED, 2)
    check_jitter(j, want_j, "fresh")
    check_noise(n, want_n, "fresh")
    assert j.device == n.device == torch.device(DEV) and j.dtype == n.dtype == torch.float32
    for R, S in ((0, 64), (5, 0), (0, 0)):
        j, n = L().train_draws(R, S, SEED, 0, device=DEV)
        assert j.shape == n.shape == (R, S)
    with pytest.raises(ValueError):
        L().train_draws(4, 4, SEED, 0, want_jitter=False, want_noise=False, device=DEV)
    with pytest.raises(ValueError):
        L().train_draws(4, 4, SEED, 0, ray_ids=torch.zeros(3, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        L().train_draws(4, 4, SEED, 0, out=(torch.zeros(4, 5, device=DEV), None))


@pytest.mark.parametrize("want", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("S", [64, 5])
def test_output_forms_and_noise_std(want, S):
    R = 257
    want_j, unit = DR.draws(R, S, SEED, 4)
    for std in (1.0, 0.5, 0.0):
        j, n = draw(R, S, SEED, 4, offset=(1 if std == 0.5 else 0), want=want, noise_std=std)
        if want[0]:
            check_jitter(j, want_j, (want, std))
        if want[1]:
            scaled = DR.draws(R, S, SEED, 4, noise_std=std, want_jitter=False)[1]
            assert np.array_equal(scaled, unit * np.float32(std))
            check_noise(n, scaled, (want, std))
            if std == 0.0:          # zeros with the unit draw's sign, as the host path's mul_ leaves them
                assert not n.any() and np.array_equal(np.signbit(n.cpu().numpy()), np.signbit(unit))


@pytest.mark.parametrize("step", [0, 1, 2 ** 32 - 1])
@pytest.mark.parametrize("seed", [SEED, 5, 0xffffffff_00000005])
def test_steps_and_seeds(step, seed):
    R, S = 65, 13
    j, n = draw(R, S, seed, step)
    want_j, want_n = DR.draws(R, S, seed, step)
    check_jitter(j, want_j, (seed, step))
    check_noise(n, want_n, (seed, step))
    if seed == 5:          # the high word of the seed and the step both count; seed and step wrap at 2^64 and 2^32
        other = draw(R, S, 0xffffffff_00000005, step)
        assert not torch.equal(j, other[0]) and not torch.equal(n, other[1])
        again = draw(R, S, seed + (1 << 64), step + (1 << 32))
        assert torch.equal(j, again[0]) and torch.equal(bits_t(n), bits_t(again[1]))


def bits_t(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return all(torch.equal(bits_t(x), bits_t(y)) for x, y in zip(a, b))


def test_ray_ids():
    R, S, step = 257, 20, 7
    whole = draw(R, S, SEED, step)
    assert same(whole, draw(R, S, SEED, step))          # two identical calls: identical bits
    # any split into calls with ray_base offsets
    for cuts in ((0, 1, 64, 257), (0, 130, 257), (0, 256, 257)):
        parts = [draw(hi - lo, S, SEED, step, ray_base=lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
        assert same(whole, [torch.cat([p[k] for p in parts]) for k in range(2)]), cuts
    # a permutation of the ids permutes the rows; repeated ids repeat rows
    perm = torch.from_numpy(np.random.RandomState(3).permutation(R).astype(np.int32)).to(DEV)
    assert same([w[perm.long()] for w in whole], draw(R, S, SEED, step, ray_ids=perm))
    rep = torch.tensor([5, 5, 200, 5, 0, 200], dtype=torch.int32, device=DEV)
    assert same([w[rep.long()] for w in whole], draw(6, S, SEED, step, ray_ids=rep))
    # ray_base = 2^32 - 3 wraps around: rows 3 ... are the ids 0 ..., rows 0 .. 2 the ids -3 .. -1 as int32
    wrapped = draw(8, S, SEED, step, ray_base=2 ** 32 - 3)
    assert same([w[:5] for w in whole], [w[3:] for w in wrapped])
    neg = torch.tensor([-3, -2, -1], dtype=torch.int32, device=DEV)
    assert same([w[:3] for w in wrapped], draw(3, S, SEED, step, ray_ids=neg))
    want_j, want_n = DR.draws(8, S, SEED, step, ray_base=2 ** 32 - 3)
    check_jitter(wrapped[0], want_j, "wrap")
    check_noise(wrapped[1], want_n, "wrap")
    # ids beyond the batch: the restatement's rows
    big = np.array([2 ** 31 - 1, -2 ** 31, 123456789, 8191 * 640 + 639], dtype=np.int32)
    got = draw(4, S, SEED, step, ray_ids=torch.from_numpy(big).to(DEV))
    want_j, want_n = DR.draws(4, S, SEED, step, ray_ids=big)
    check_jitter(got[0], want_j, "big ids")
    check_noise(got[1], want_n, "big ids")


# ---- 2. the renderer --------------------------------------------------------------------------------------------------------------------
OUT_KEYS = ("color", "disp_map", "acc_map", "depth_map", "weights", "z_vals")


@pytest.fixture(params=[False, True], ids=["plain", "poisoned"])
def scratch(request, monkeypatch):
    if request.param:
        monkeypatch.setenv("DSN_POISON_SCRATCH", "1")
    else:
        monkeypatch.delenv("DSN_POISON_SCRATCH", raising=False)


@pytest.fixture(scope="module")
def g():
    return load("small_train_grads")


def renderer(g, draws="device", seed=SEED, step=0):
    from cases import make_renderer
    r = make_renderer(g)
    r.cfg.MODEL.raw_noise_std = float(g["raw_noise_std"])
    r.train()
    assert r.draws == "host" and r.draw_state() == {"seed": 0, "step": 0} and r.last_draws is None
    r.draws = draws
    r.seed_draws(seed, step)
    return r


def batch(g, rows=None, **extra):
    from cases import make_batch
    b = make_batch(g)
    if rows is not None:
        for k in ("ray_o", "ray_d", "near", "far"):
            b[k] = b[k][:, rows].clone()
    b.update(extra)
    return b


def step_of(r, g, b=None, backward=False, rows=None):
    """one train-mode render (and, asked for, the reference's loss and backward) -> ({output: tensor}, {parameter: gradient})"""
    from cases import reference_loss
    out = r.render(b if b is not None else batch(g))["coarse"]
    keep = {k: out[k].detach().clone() for k in OUT_KEYS}
    grads = {}
    if backward:
        sel = slice(None) if rows is None else (rows.numpy() if torch.is_tensor(rows) else rows)
        loss = reference_loss(out, torch.from_numpy(g["target_rgb"][sel]).cuda(), torch.from_numpy(g["occupancy"][sel]).cuda())
        r.net.zero_grad()
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in r.net.named_parameters()}
    return keep, grads


def differing(a, b):
    return {k: int((bits_t(a[k]) != bits_t(b[k])).sum()) for k in a if not torch.equal(bits_t(a[k]), bits_t(b[k]))}


def device_and_host_step(g, rows=None, host_runs=1):
    """one step with draws = "device" and the same step on the host path of a second renderer (of `host_runs` fresh renderers) whose
    _draws is replaced by a function returning the device step's last_draws -> (device renderer, outputs and gradients of the
    device step, [outputs and gradients of each host step])"""
    rd = renderer(g, step=5)
    out_d, grad_d = step_of(rd, g, batch(g, rows=rows), backward=True, rows=rows)
    jitter, noise = rd.last_draws
    hosts = []
    for _ in range(host_runs):
        rh = renderer(g, draws="host")
        rh._draws = lambda R_, S_: (jitter, noise)
        hosts.append(step_of(rh, g, batch(g, rows=rows), backward=True, rows=rows))
        assert rh.draw_state() == {"seed": SEED, "step": 0} and rh.last_draws[0] is jitter and rh.last_draws[1] is noise
    return rd, (out_d, grad_d), hosts


def test_device_path_changes_only_the_source_of_the_draws(g, scratch):
    """every output of a train-mode render with draws = "device" against a render on the host path whose _draws is replaced by a
    function returning the device step's last_draws: bit for bit.  The draws themselves are the restatement's at (seed, step), with
    the rays' ids 0 .. R - 1; the step counter advances by one; nothing of the host path's staging is set up."""
    R, S = g["ray_o"].shape[0], int(g["S"])
    rd, (out_d, _), [(out_h, _)] = device_and_host_step(g)
    jitter, noise = rd.last_draws
    assert rd.draw_state() == {"seed": SEED, "step": 6}
    want_j, want_n = DR.draws(R, S, SEED, 5, noise_std=float(g["raw_noise_std"]))
    check_jitter(jitter, want_j, "renderer")
    check_noise(noise, want_n, "renderer")
    assert not hasattr(rd, "_draw_ring")          # no page-locked staging ring: nothing came from the host
    bad = differing(out_d, out_h)
    print("differing output words:", bad)
    assert not bad, bad


GRAD_RAYS = 4          # x 16 samples = 64 rows: one workgroup's share in every sum of the backward (see the test below)


def test_device_path_gradients_are_bit_identical(g, scratch):
    """the gradients after backward() of the same two steps, bit for bit in all 33 tensors - on a batch of the GRAD_RAYS rays with the
    largest opacity, because that is where the training backward is itself reproducible.  It sums three tensors with floating-point
    atomics across workgroups (lights_encoding.0's weight and bias in the exact-fp32 product k_t_wgrad, whose workgroups own at least
    64 rows each; density_net.0.weight in k_tangent16's column sum), so at the fixture's 64 rays x 16 samples two runs of ONE path with
    identical draws already differ there.  Measured on the MI355X at 64 x 16, four repetitions each, differing words and relative L2:
        device against host:   lights_encoding.0.weight 416 - 440 words, 5.5e-8 - 5.9e-8;  .bias 46 - 56 words, 4.9e-8 - 6.3e-8
        host against host:     lights_encoding.0.weight 309 - 520 words, 5.1e-8 - 7.0e-8;  .bias 22 - 65 words, 3.5e-8 - 8.2e-8;
                               density_net.0.weight 6 words, 5.7e-9, in two of the four
        device against device: 475 / 55 / 6 words, 7.0e-8 / 5.5e-8 / 5.7e-9
    with the other 30 tensors and every output of the forward pass bit-identical in all of them.  With 64 rows every such sum has one
    contribution per word, whatever the order the workgroups arrive in.  The test first shows that: two runs of the host path give the
    same bits (otherwise the comparison would say nothing about the draws); then the device step's gradients equal them."""
    rows = torch.from_numpy(np.sort(np.argsort(-g["render:acc_map"], kind="stable")[:GRAD_RAYS]))
    assert GRAD_RAYS * int(g["S"]) <= 64
    _, (_, grad_d), [(_, grad_h), (_, grad_h2)] = device_and_host_step(g, rows=rows, host_runs=2)
    assert set(grad_d) == set(grad_h) == set(grad_h2) and len(grad_d) == 33
    live = [k for k, v in grad_h.items() if bool(v.any())]
    print(len(live), "of 33 gradients are not all zero")
    # (not a check of zeros against zeros, least of all in the three tensors in question)
    assert {"lighting_mlp.lights_encoding.0.weight", "lighting_mlp.lights_encoding.0.bias", "nerf.density_net.0.weight"} <= set(live)
    bad = differing(grad_h, grad_h2)
    assert not bad, ("the host path does not reproduce its own gradients at this size", bad)
    bad = differing(grad_d, grad_h)
    print("differing gradient words:", bad)
    assert not bad, bad


def test_draw_state_resumes_a_run(g, scratch):
    """seed_draws and three steps against a fresh renderer that loads the draw state saved after step one and runs two more"""
    r1 = renderer(g, seed=77, step=2 ** 32 - 2)          # (the step counter wraps at 2^32 on the way)
    outs, states, draws = [], [], []
    for _ in range(3):
        outs.append(step_of(r1, g)[0])
        states.append(dict(r1.draw_state()))
        draws.append(r1.last_draws)
    assert [s["step"] for s in states] == [2 ** 32 - 1, 0, 1] and all(s["seed"] == 77 for s in states)
    assert not same(draws[0], draws[1]) and not same(draws[1], draws[2])
    r2 = renderer(g, seed=1, step=1)
    r2.load_draw_state(states[0])
    for k in (1, 2):
        out = step_of(r2, g)[0]
        assert same(r2.last_draws, draws[k]) and not differing(out, outs[k]), k
    assert r2.draw_state() == states[2]


def test_ray_ids_make_a_batch_splittable(g, scratch):
    """a batch that carries ray_ids, rendered whole and in two halves at the same step: the halves of the whole.  int64 and int32 ids,
    [1, R]; and ray_base offsets do the same for ids that are consecutive."""
    R = g["ray_o"].shape[0]
    ids = torch.from_numpy(((np.arange(R, dtype=np.int64) * 2654435761 + 17) % (1 << 20))).to(DEV)[None]
    r = renderer(g, step=9)
    whole = step_of(r, g, batch(g, ray_ids=ids))[0]
    whole_draws = r.last_draws
    assert r.draw_state()["step"] == 10
    for dtype in (torch.int64, torch.int32):
        for rows in (slice(0, 29), slice(29, R)):
            r.seed_draws(SEED, 9)
            part = step_of(r, g, batch(g, rows=rows, ray_ids=ids[:, rows].to(dtype)))[0]
            assert same(r.last_draws, [w[rows] for w in whole_draws]), (dtype, rows)
            bad = differing(part, {k: v[rows] for k, v in whole.items()})
            assert not bad, (dtype, rows, bad)
    r.seed_draws(SEED, 9)
    step_of(r, g)
    plain = r.last_draws
    r.seed_draws(SEED, 9)
    step_of(r, g, batch(g, rows=slice(29, R), ray_base=29))
    assert same(r.last_draws, [w[29:] for w in plain])
    with pytest.raises(ValueError):
        r.render(batch(g, ray_ids=ids[:, :5]))


def test_host_generator_and_host_path_are_untouched(g, scratch):
    """a "device" step leaves the CPU generator's state alone; a "host" step gives the same bits before and after "device" steps on
    the same renderer; render_view gives the same bits before and after"""
    from cases import make_batch
    gv = load("small_view")
    r = renderer(g, draws="host")

    def view():
        r.eval()
        b = make_batch(gv)
        b["img"] = torch.zeros(1, int(gv["H"]), int(gv["W"]), 3, dtype=torch.float64)
        b["mask_at_box"] = torch.from_numpy(gv["mask_at_box"])[None]
        out = {k: v.clone() for k, v in r.render_view(b).items() if torch.is_tensor(v)}
        r.train()
        return out

    view_before = view()
    torch.manual_seed(1234)
    host_before = step_of(r, g)[0]
    host_draws = r.last_draws
    r.draws = "device"
    state = torch.get_rng_state()
    for _ in range(2):
        step_of(r, g, backward=True)
    # the stage calls in train mode draw from the rule at the current step, without advancing it and without the CPU generator
    b = batch(g)
    R, S = g["ray_o"].shape[0], int(g["S"])
    with torch.no_grad():
        pts, z = r.get_sampling_points(b["ray_o"], b["ray_d"], b["near"], b["far"], b["xyz"])
    assert torch.equal(state, torch.get_rng_state()) and r.draw_state() == {"seed": SEED, "step": 2}
    assert tuple(z.shape) == (1, R, S)
    want_j, want_n = DR.draws(R, S, SEED, 2, noise_std=float(g["raw_noise_std"]))
    j, n = r._device_draws(R, S)
    check_jitter(j, want_j, "stage jitter")
    check_noise(n, want_n, "stage noise")
    assert torch.equal(state, torch.get_rng_state())
    r.draws = "host"
    torch.manual_seed(1234)
    host_after = step_of(r, g)[0]
    assert same(host_draws, r.last_draws) and not differing(host_before, host_after)
    bad = differing(view_before, view())
    assert not bad, bad
    r.draws = "gpu"
    with pytest.raises(ValueError):
        r.render(batch(g))


def test_stage_calls_draw_from_the_rule(scratch, monkeypatch):
    """train-mode render_rays / batchify_pts with draws = "device": the noise handed to the compositor is the rule's at the current
    step (ids from ray_base where the batch carries one), the step does not advance, the CPU generator is not used, and two calls
    give the same bits"""
    import dsnerf_amd
    from cases import make_batch, make_renderer
    gs = load("small_train")
    r = make_renderer(gs, "small_train")
    r.train()
    r.draws = "device"
    r.seed_draws(SEED, 41)
    b = make_batch(gs)
    R, S = gs["ray_o"].shape[0], int(gs["S"])
    dirs = np.repeat(gs["ray_d"][:, None, :], S, 1)
    pts6 = torch.from_numpy(np.concatenate([gs["pts"].reshape(-1, S, 3), gs["x_c"].reshape(-1, S, 3)], -1))
    rays6 = torch.from_numpy(np.concatenate([dirs, gs["ray_d_can"].reshape(-1, S, 3)], -1))
    b["canonical_model"], b["face_idx"] = r.canonical_model, r.face_idx
    b["transparent_mask"] = torch.from_numpy(gs["transparent"]).reshape(-1, S)
    fi = torch.full((R, S), int(gs["frame"]))
    seen = []
    composite = dsnerf_amd._lib.composite
    monkeypatch.setattr(dsnerf_amd._lib, "composite", lambda *a: (seen.append(a[5]), composite(*a))[1])
    state = torch.get_rng_state()
    outs = []
    with torch.no_grad():
        for base in (None, None, 1000):
            if base is not None:
                b["ray_base"] = base
            outs.append(r.batchify_pts(pts6, rays6, torch.from_numpy(gs["z_vals"]), fi, batch_info=b))
    assert torch.equal(state, torch.get_rng_state()) and r.draw_state() == {"seed": SEED, "step": 41}
    assert len(seen) == 3 and all(n is not None and tuple(n.shape) == (R, S) for n in seen)
    std = float(r.cfg.MODEL.raw_noise_std)
    check_noise(seen[0], DR.draws(R, S, SEED, 41, noise_std=std, want_jitter=False)[1], "stage noise")
    check_noise(seen[2], DR.draws(R, S, SEED, 41, ray_base=1000, noise_std=std, want_jitter=False)[1], "stage noise, ray_base")
    assert torch.equal(bits_t(seen[0]), bits_t(seen[1])) and not differing(outs[0], outs[1])
    assert differing(outs[0], outs[2])          # other ids, other noise, other pixels
    r.eval()
    with torch.no_grad():
        r.batchify_pts(pts6, rays6, torch.from_numpy(gs["z_vals"]), fi, batch_info=b)
    assert seen[3] is None          # eval mode draws nothing
