"""GPU: the state a Renderer keeps BETWEEN calls.  Call B on a renderer that has just done A must return what B returns on a renderer
that has done nothing ("a call's result is a function of its arguments").

call_sequence_ops.py holds the catalogue: the output operations (render, the view calls, the training steps, the stage calls, the mesh
calls, the metrics, the codecs) and the state changes (the pose as a new tensor / in place / at the freed address, either parameter
set loaded, train / eval, lazy lists off / on, the density screen with its audit on / off - each sets a state, none toggles), on two bodies - the 162-vertex one and the 6890-vertex one, whose
pose tensor (82 KB) goes through the staging ring, whose sampler takes the vertex-slice path and whose 128 x 128 view reaches the fused
classification.  (The relighting sweep and the maps need S = 64 or 128: they run on the full body only, the small one renders S = 16.)
Everything here runs with DSN_POISON_SCRATCH=1: a new workspace is 0xFF bytes, never zeros.

  fresh table    every (operation, pose, parameter set) on a newly constructed Renderer: what the call returns "from nothing"
  pair walk      ONE long-lived renderer per body runs an Eulerian circuit of the complete digraph (with loops) of the output operations
                 - every ordered pair consecutive exactly once, N^2 + 1 steps - then every state change directly in front of every
                 output operation.  The walk is cut into segments of SEGMENT steps (a test function each, the renderer carried from one
                 to the next; a segment starts with the step the previous one ended with, so no pair is lost at a cut); every segment
                 asserts that the pairs it RAN are the ones it was to run, and the last test that all of them were run.
  seeded walks   three walks of 40 steps drawn from all operations, on the same long-lived renderer
  early stop     on the w4 parameters the history dependence is by design: a sliced frame equals the sliced frame of a fresh renderer
                 that rendered the same probe frame first, stays within the bound its last_frame_info reports, and a parameter change
                 makes the next eval frame a probe again - in either direction
  sensitivity    with Renderer._is_frame_src comparing data_ptr() only (the first bug of this class the project had), the in-place pose
                 update is caught

The rule of comparison (call_sequence_ops.difference): bit for bit, as int32 words - NaN in disp is legitimate.  A quantity takes a
tolerance only where two FRESH renderers already disagree, and then the one the suite already has: dsn_image_psnr's four keys 1e-12
relative (tests/test_gpu_lpips.py), and the gradient tensors of call_sequence_ops.LOOSE_GRADS - the head products that end in float
atomics: 3 tensors on the small body, 8 on the full one - FLOOR = 2e-6 relative L2 (tests/test_gpu_train.py); every other gradient,
the trunk's included (tests/test_gpu_train_bits.py), stays bit-exact.  test_two_fresh_renderers_agree prints what two fresh renderers differ by, key by key:
that is the evidence for those two and would show a third.  A difference seen only long-lived-against-fresh is the finding."""
import gc
import random

import pytest
import torch

import call_sequence_ops as C
from test_gpu_train import FLOOR

pytestmark = pytest.mark.gpu
BODIES = ("small", "full")
SEGMENT = 40                      # steps of the pair walk per test function
SEEDS = (101, 202, 303)
WALK_STEPS = 40
STOP_EPS = 2.0 ** -20             # the cap of _lib.early_stop_eps (tests/test_gpu_round2.py)


@pytest.fixture(scope="module", autouse=True)
def poisoned():
    mp = pytest.MonkeyPatch()
    mp.setenv("DSN_POISON_SCRATCH", "1")
    yield
    mp.undo()
    # the long-lived renderers end with the module (tests after this one count the Renderer objects alive in the process)
    _LIVE.clear()
    _FRESH.clear()
    gc.collect()


# ---- the plan (host only: names, no body is built here) -------------------------------------------------------------------------
def circuit(bname):
    return C.euler_circuit(list(C.output_ops(bname)))


def state_section(bname):
    """every state change directly in front of every output operation"""
    return [x for s in C.STATE_OPS for o in C.output_ops(bname) for x in (s, o)]


def segments(bname):
    """the pair walk cut into pieces: the circuit in runs of SEGMENT steps that overlap by one, then the state section in whole
    (state change, operation) couples"""
    walk, out = circuit(bname), []
    i = 0
    while i < len(walk) - 1:
        out.append(walk[i:i + SEGMENT + 1])
        i += SEGMENT
    sec = state_section(bname)
    step = SEGMENT - SEGMENT % 2
    out += [sec[i:i + step] for i in range(0, len(sec), step)]
    return out


def planned(bname, seq):
    """(output pairs, (state change, output operation) couples) consecutive in a sequence"""
    outs = C.output_ops(bname)
    pairs = {(a, b) for a, b in C.pairs_of(seq) if a in outs and b in outs}
    couples = {(a, b) for a, b in C.pairs_of(seq) if a in C.STATE_OPS and b in outs}
    return pairs, couples


SEGMENT_IDS = [(b, k) for b in BODIES for k in range(len(segments(b)))]


# ---- module state: the fresh table, the long-lived renderers, what ran -------------------------------------------------------------
_FRESH, _LIVE = {}, {}
RAN = {b: {"segments": set(), "pairs": set(), "couples": set(), "frames": []} for b in BODIES}
COUNTS = {"steps": 0, "comparisons": 0, "tensors": 0}


def fresh(bname, name, pose, params):
    key = (bname, name, pose, params)
    if key not in _FRESH:
        _FRESH[key] = C.fresh_result(C.body(bname), name, pose, params)
    return _FRESH[key]


def live(bname):
    if bname not in _LIVE:
        b = C.body(bname)
        _LIVE[bname] = (C.new_renderer(b), C.new_state(b))
    return _LIVE[bname]


def run_steps(bname, r, state, seq):
    """run a sequence; one record per step: (step name, the step before it, (pose, params) before and after the step, result or None)"""
    b = C.body(bname)
    records, prev = [], None
    for name in seq:
        before = (state["pose"], state["params"])
        res = C.any_op(b, name)(r, state)
        frame = name in C.EVAL_FRAME_OPS
        records.append({"name": name, "prev": prev, "before": before, "at": (state["pose"], state["params"]), "result": res,
                        "state": C.describe(state), "screened": bool(r.last_frame_info["density_screen"]) if frame else None,
                        "lazy": bool(r.scene.lazy) if frame else None})
        prev = name
    torch.cuda.synchronize()
    COUNTS["steps"] += len(seq)
    return records


def explain(bname, records, i, diff):
    """the failure message: operation, the step before it, the state, the first differing key, the count - and whether [previous,
    operation] alone, once, on a fresh renderer shows the same difference"""
    rec = records[i]
    key, n, what = diff
    msg = ["%s body: `%s` directly after `%s` (%s) differs from the fresh table: first key %r, %s"
           % (bname, rec["name"], rec["prev"], rec["state"], key, what)]
    if rec["prev"] is not None:
        start = records[i - 1]["before"]
        alone = C.fresh_result(C.body(bname), rec["name"], start[0], start[1], before=(rec["prev"],))
        d = C.first_difference(alone, fresh(bname, rec["name"], *rec["at"]), bname)
        msg.append("[%s, %s] alone on a fresh renderer %s" % (rec["prev"], rec["name"], "does NOT show it: longer history is needed"
                                                             if d is None else "shows it too: first key %r, %s" % (d[0], d[2])))
    msg.append("steps so far: " + " ".join(x["name"] for x in records[:i + 1]))
    return "\n".join(msg)


def check(bname, records):
    for i, rec in enumerate(records):
        if rec["result"] is None:
            continue
        want = fresh(bname, rec["name"], *rec["at"])
        COUNTS["comparisons"] += 1
        COUNTS["tensors"] += len(want)
        d = C.first_difference(rec["result"], want, bname)
        if d is not None:
            pytest.fail(explain(bname, records, i, d))


def run_segment(bname, k):
    seq = segments(bname)[k]
    r, state = live(bname)
    records = run_steps(bname, r, state, seq)
    ran = planned(bname, [x["name"] for x in records])
    assert ran == planned(bname, seq)                      # what ran is what this segment was to run
    check(bname, records)
    RAN[bname]["segments"].add(k)
    RAN[bname]["pairs"] |= ran[0]
    RAN[bname]["couples"] |= ran[1]
    # what the eval frames directly behind a state change ran with: (state change, operation, parameter set, screen engaged, lazily set)
    RAN[bname]["frames"] += [(x["prev"], x["name"], x["at"][1], x["screened"], x["lazy"]) for x in records
                             if x["prev"] in C.STATE_OPS and x["screened"] is not None]


# ---- 1. the fresh table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(C.FAMILIES))
@pytest.mark.parametrize("params", C.PARAMS)
@pytest.mark.parametrize("bname", BODIES)
def test_fresh_table(bname, params, family):
    """every (operation, pose) of a parameter set on its own new Renderer, a family of operations at a time; the operations that exist
    to reach a path assert that they do (view_fused: n >= 1 << 20, the staging ring's 64 KB), and nothing in the table is empty"""
    have = dict(C.output_ops(bname), **C.EXTRA_OPS)
    names = [n for n in C.FAMILIES[family] if n in have]
    assert names
    for name in names:
        for pose in (0, 1):
            res = fresh(bname, name, pose, params)
            assert res and all(torch.is_tensor(v) and v.numel() > 0 for v in res.values()), (name, pose)
    b = C.body(bname)
    assert (b.V >= 512) == (bname == "full")               # (the sampler's vertex-slice path: the full body only)
    other = C.PARAMS[1 - C.PARAMS.index(params)]
    for name in [n for n in ("render", "view", "views", "train_host", "w2l", "density_grid") if n in names]:
        # the poses are told apart, and - where the parameters enter at all - the parameter sets
        assert C.first_difference(fresh(bname, name, 0, params), fresh(bname, name, 1, params), bname) is not None, name
        if name != "w2l":
            assert C.first_difference(fresh(bname, name, 0, params), fresh(bname, name, 0, other), bname) is not None, name
    if bname == "full" and params == "w4" and family == "meshes":
        assert "no_surface" not in fresh(bname, "extract_mesh", 0, params)      # (the converged field has a surface to extract)


@pytest.mark.parametrize("params", C.PARAMS)
@pytest.mark.parametrize("bname", BODIES)
def test_two_fresh_renderers_agree(bname, params):
    """a second fresh renderer per operation (pose 0) against the table, under the same rule; prints, key by key, what the two differ
    by in bits - the fresh-against-fresh evidence behind every quantity that takes a tolerance.  Both directions are asserted: a key
    that differs in bits has a tolerance, and of the gradients that have one, the first lighting layer's weight - 285 to 830 words
    in every run recorded - differs here too (the rarer ones, one-element biases among them, are listed when they did not: a
    tolerance that no run needs any more shows up in that list run after run)"""
    assert C.FLOOR == FLOOR
    loose, tolerant = {}, set()
    for name in list(C.output_ops(bname)) + list(C.EXTRA_OPS):
        for pose in (0,):
            a, b = fresh(bname, name, pose, params), C.fresh_result(C.body(bname), name, pose, params)
            assert C.first_difference(b, a, bname) is None, (name, pose, C.first_difference(b, a, bname))
            for k in a:
                if C.tolerance_of(k, bname) is not None:
                    tolerant.add(k)
                n = int((C.words(a[k]) != C.words(b[k].to(a[k].device))).sum())
                if n:
                    rel = float((a[k].double() - b[k].double()).norm() / a[k].double().norm().clamp_min(1e-300))
                    old = loose.get(k, (0, 0.0, 0))
                    loose[k] = (max(old[0], n), max(old[1], rel), old[2] + 1)
                    assert C.tolerance_of(k, bname) is not None, (name, pose, k, n, rel)
    assert tolerant == set(C.PSNR_KEYS) | {"grad:" + g for g in C.LOOSE_GRADS[bname]}
    assert "grad:lighting_mlp.lights_encoding.0.weight" in loose
    print("%s body, %s parameters: fresh against fresh, keys that differ in bits (most words, largest relative L2, calls in which they differed): %s; "
          "tolerant keys that did not differ in this run: %s" % (bname, params, loose or "none", sorted(tolerant - set(loose)) or "none"))


# ---- 2. the pair walk --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bname,k", SEGMENT_IDS, ids=["%s-%02d" % s for s in SEGMENT_IDS])
def test_pair_walk(bname, k):
    run_segment(bname, k)


@pytest.mark.parametrize("bname", BODIES)
def test_pair_walk_covered_every_ordered_pair(bname):
    """the pairs the segments RAN are all N^2 ordered pairs of output operations, and every state change ran directly in front of
    every output operation (segments not run yet - a selection with -k - are run here)"""
    for k in range(len(segments(bname))):
        if k not in RAN[bname]["segments"]:
            run_segment(bname, k)
    outs = list(C.output_ops(bname))
    assert len(circuit(bname)) == len(outs) ** 2 + 1
    assert RAN[bname]["pairs"] == {(a, b) for a in outs for b in outs}
    assert RAN[bname]["couples"] == {(s, o) for s in C.STATE_OPS for o in outs}
    # the state changes set a state, they do not toggle one: every operation follows each direction - and they took effect.  Every
    # eval frame directly behind lazy_off was set with every cell's lists, behind lazy_on lazily; no frame behind screen_off ran the
    # screen; behind screen_on the frames of the default parameters did (the walk loads them last; w4 calibrates the screen unsafe)
    frames = RAN[bname]["frames"]
    eval_ops = [o for o in outs if o in C.EVAL_FRAME_OPS]
    for s, want in (("lazy_off", False), ("lazy_on", True)):
        got = {o: lazy for p, o, _, _, lazy in frames if p == s}
        assert got == {o: want for o in eval_ops}, (s, got)
    assert {o for p, o, _, on, _ in frames if p == "screen_off" and not on} == set(eval_ops)
    behind_on = {o: (params, on) for p, o, params, on, _ in frames if p == "screen_on"}
    assert set(behind_on) == set(eval_ops) and all(params == "default" for params, _ in behind_on.values()), behind_on
    engaged = sorted(o for o, (_, on) in behind_on.items() if on)
    assert engaged == sorted(eval_ops), "the density screen did not engage behind screen_on for %s" % sorted(set(eval_ops) - set(engaged))
    _, state = live(bname)
    print("%s body: %d output operations, %d ordered pairs, %d (state change, operation) couples in %d segments; address reused %d times; "
          "so far %d steps, %d results of %d tensors compared" % (bname, len(outs), len(RAN[bname]["pairs"]), len(RAN[bname]["couples"]),
                                                                   len(segments(bname)), state.get("address_reused", 0), COUNTS["steps"],
                                                                   COUNTS["comparisons"], COUNTS["tensors"]))


# ---- 3. seeded walks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("bname", BODIES)
def test_seeded_walk(bname, seed):
    names = list(C.output_ops(bname)) + list(C.STATE_OPS)
    rng = random.Random(seed)
    seq = [rng.choice(names) for _ in range(WALK_STEPS)]
    r, state = live(bname)
    check(bname, run_steps(bname, r, state, seq))


# ---- 4. early stop: the one designed history dependence ---------------------------------------------------------------------------
def _frame(r, state, name):
    """an eval operation and the last_frame_info it left"""
    res = C.any_op(state["body"], name)(r, state)
    return res, dict(r.last_frame_info)


def _replay(b, mode, probe_pose, state, name):
    """the documented minimal history on a fresh renderer: the probe frame (its statistics read), then the frame"""
    r = C.new_renderer(b, "w4", early_stop=mode)
    _frame(r, C.new_state(b, probe_pose, "w4"), "view_device")
    r._read_stop_probe(wait=True)
    return _frame(r, C.new_state(b, state["pose"], "w4"), name)


def _within_its_bound(got, one_pass, info, b):
    """a sliced frame against the one-pass frame: the colour bound its own last_frame_info reports (+ fp32 summation order, as
    tests/test_gpu_round2.py::_assert_stop_bound grants it), acc and depth as that function has them"""
    cmax = max(1.0, float(one_pass["coarse_color"].abs().max()))
    assert float((got["coarse_color"] - one_pass["coarse_color"]).abs().max()) <= info["early_stop_bound_abs"] + 2e-6 * cmax
    assert info["early_stop_bound_abs"] <= 0.5e-4 * max(1.0, info["early_stop_colour_scale"]) * (1 + 1e-6)
    assert float((got["coarse_acc"] - one_pass["coarse_acc"]).abs().max()) <= 2 * STOP_EPS
    far = max(float(b.view(p, b.view_hw)[0]["far"].max()) for p in (0, 1))
    assert float((got["coarse_depth"] - one_pass["coarse_depth"]).abs().max()) <= 2 * STOP_EPS * far


@pytest.mark.parametrize("mode", ["auto", True])
def test_early_stop_walk(mode):
    """w4 on the full body, early_stop = "auto" / True: probe, sliced frames of both poses between a sweep, the maps and frames in
    flight, then the parameters changed and changed back"""
    b = C.body("full")
    r, state = C.new_renderer(b, "w4", early_stop=mode), C.new_state(b, 0, "w4")
    _, info = _frame(r, state, "view_device")
    assert info["early_stop"] is False                                   # the first eval frame of a parameter version: the probe
    r._read_stop_probe(wait=True)
    plan = r.net.packed(r.device).early_stop
    assert plan is not None and plan["finite"] and (plan["usable"] or mode is True), plan
    probe_pose = 0
    sliced = 0
    for name in ("view_device", "view_lights", "pose_new", "view_device", "view_maps", "views", "pose_in_place", "view_device"):
        if name in C.STATE_OPS:
            C.STATE_OPS[name](r, state)
            continue
        got, info = _frame(r, state, name)
        assert info["early_stop"] is True and not info.get("rendered_again_in_one_pass"), (name, info)
        want, winfo = _replay(b, mode, probe_pose, state, name)
        d = C.first_difference(got, want, "full")
        assert d is None, "early_stop = %r: `%s` (%s) differs from probe + frame on a fresh renderer: %r" % (mode, name, C.describe(state), d)
        assert winfo["early_stop_colour_scale"] == info["early_stop_colour_scale"]
        if name == "view_device":
            _within_its_bound(got, fresh("full", "view_device", state["pose"], "w4"), info, b)
            sliced += 1
    assert sliced == 3
    # a parameter change: the next eval frame is a probe again - and so is the next one after changing BACK (the plan is keyed by
    # packed.generation: the first w4 plan is not resurrected)
    for back in (False, True):
        C.STATE_OPS["params_w4" if back else "params_default"](r, state)
        assert r.net.packed(r.device).early_stop is None
        got, info = _frame(r, state, "view_device")
        assert info["early_stop"] is False, (back, info)
        r._read_stop_probe(wait=True)
        probe_pose = state["pose"]
    got, info = _frame(r, state, "view_device")
    assert info["early_stop"] is True
    want, _ = _replay(b, mode, probe_pose, state, "view_device")
    assert C.first_difference(got, want, "full") is None, C.first_difference(got, want, "full")
    _within_its_bound(got, fresh("full", "view_device", state["pose"], "w4"), info, b)


# ---- 5. sensitivity ------------------------------------------------------------------------------------------------------------------
def _keyed_on_address(self, xyz):
    """the mutant: the posed mesh keyed on data_ptr() alone (what the project once had)"""
    src = self._frame_src
    return src is not None and src[0]() is not None and src[0]().data_ptr() == xyz.data_ptr()


def test_walk_catches_a_posed_mesh_keyed_on_its_address(monkeypatch):
    """[operation, pose updated in place, operation]: the real code returns the fresh table's entries; with _is_frame_src comparing
    addresses the second call keeps the old posed mesh and differs.  Python only: wrong values, nothing that could fault.
    The operation is w2l_without_lbs, the call the bug was found in.  render_view cannot show this mutant: it sets its frame on every
    call and never asks _is_frame_src (the second half of the sequence holds that); the walks run every operation directly after the
    in-place update, so whichever operation trusts the key is met."""
    import dsnerf_amd
    b = C.body("small")
    seq = ["w2l", "pose_in_place", "w2l", "pose_in_place", "view", "pose_in_place", "view"]

    def differences():
        r, state = C.new_renderer(b), C.new_state(b)
        recs = run_steps("small", r, state, seq)
        return [(x["name"], C.first_difference(x["result"], fresh("small", x["name"], *x["at"]), "small")) for x in recs if x["result"] is not None]

    assert all(d is None for _, d in differences())
    monkeypatch.setattr(dsnerf_amd.Renderer, "_is_frame_src", _keyed_on_address)
    got = differences()
    assert got[0][1] is None and got[1][1] is not None, got            # the call after the in-place update kept the old pose
    assert got[2][1] is None and got[3][1] is None, got                # render_view sets its own frame
