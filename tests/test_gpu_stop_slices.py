"""DSN_EARLY_STOP's kernels (csrc/dsn_geom.hip: k_slice_bucket, k_advance_T<G>, k_slice_alive<LC>, k_cull_lit, k_stop_stats) slice by
slice against tests/stop_slices_restate.py, through _lib.render_rays.

Per case: a one-pass frame (DSN_STOP_STATS, no screen) and a sliced frame on a fresh workspace; per-sample sigma / transparent / colour
are read from both workspaces (helpers.workspace_arrays).  The restatement is fed the ONE-PASS device sigma and says, per ray and
slice, certainly alive / certainly dead / undetermined; the sliced frame must have the one-pass density bit for bit wherever its ray is
alive and exactly 0 wherever it is dead, its counters must be the restated counts, and the one-pass frame's statistics the restated
statistics.  Frames: the reference's golden rays of full_eval_w4 / full_eval_w3 and a synthetic 67 x 67 frame per weight set
(R = 4489: no multiple of 64, a tail workgroup in every k_advance_T<G>; R x 1 > 2048: several workgroups in the list kernels even for
slices of one sample), at S = 24, 64, 100, 128 - at most 4489 x 128 = 0.57 M samples.  Slicings: stop_slices_restate.SLICINGS - every G of
k_advance_T, ragged last slices, a single slice.

DSN_STOP_ADVANCE=list (read once per process) runs in a child process and must reproduce the default mode bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import stop_slices_restate as SR
from helpers import load, state, workspace_arrays

pytestmark = pytest.mark.gpu
HW = 67
FRAMES = ["golden_w4", "golden_w3", "synth_w4", "synth_w3"]
CNT_FLAGGED = 20              # = DSN_CNT_FLAGGED (csrc/dsn_api.hip)
IDS = [SR.slicing_id(s) for s in SR.SLICINGS]
_SETUP = {}


def setup(frame):
    """renderer (frame state set, density screen off) and device rays of a frame - built once per module"""
    if frame not in _SETUP:
        from test_gpu_render import make_batch, make_renderer
        from test_gpu_round2 import full_frame, overflowing_state, renderer_with
        kind, w = frame.split("_")
        if kind == "golden":
            g = load("full_eval_" + w)
            r = make_renderer(g, "full_eval_" + w, density_screen=False)
            batch = make_batch(g)
        else:
            canon, faces, batch = full_frame(hw=HW)
            sd = {"overflow": lambda: overflowing_state("nerf.stage1.4"), "overflowdense": dense_overflowing_state}.get(w, lambda: state("x_" + w))()
            r = renderer_with(sd, canon, faces, density_screen=False)
        r.eval()
        r._set_frame(batch)
        dev = lambda k: r._dev(batch[k][0]).clone()      # noqa: E731
        _SETUP[frame] = (r, dev("ray_o"), dev("ray_d"), dev("near"), dev("far"))
    return _SETUP[frame]


def render(frame, S, **kw):
    from dsnerf_amd import _lib
    r, o, d, near, far = setup(frame)
    ws = _lib.RenderWorkspace(r.device)                  # fresh: sized with the DSN_STOP_SLICE in force now
    out = _lib.render_rays(r.scene, r.net.packed(r.device), ws, o, d, near.clone(), far.clone(), S, r._t_vals(S), screen=False, **kw)
    torch.cuda.synchronize()
    R = o.shape[0]
    a = workspace_arrays(ws, R * S)
    res = {"sigma": a["sigma"].cpu().numpy().reshape(R, S), "transparent": a["transparent"].cpu().numpy().reshape(R, S) != 0,
           "colour": a["colour"].cpu().numpy().reshape(R, S, 3), "weights": out["weights"].cpu().numpy(),
           "z": out["z_vals"].cpu().numpy(), "d": d.cpu().numpy(), "counts": ws.buf[:1024].view(torch.int32).cpu().numpy().copy(),
           "stats": _lib.read_stop_stats(ws), "ws": ws}
    return res


def run_case(frame, sl):
    """the one-pass frame with statistics, the colour scale as the callers set it, the sliced frame.  DSN_STOP_SLICE is the caller's."""
    from dsnerf_amd import _lib
    S, kind, v = sl
    r = setup(frame)[0]
    R = setup(frame)[1].shape[0]
    pk = r.net.packed(r.device)
    pk.set_early_stop_colour_scale(1.0)                  # (every case starts from the unmeasured scale: the cases do not depend on their order)
    one = render(frame, S, stop_stats=True)
    one["Lu"] = _lib.stop_slice_len(R, S)
    one["hist"], one["Lh"] = _lib.read_stop_hist(one.pop("ws"), R, S)
    cm = one["stats"]["colour_max"]
    assert cm == cm and cm != float("inf")
    want = _lib.EARLY_STOP_COLOUR_HEADROOM * cm
    if want > pk.colour_scale:
        pk.set_early_stop_colour_scale(want)
    eps = SR.eps_scaled(S, pk.colour_scale)
    assert float(eps) == _lib.early_stop_eps(S, pk.colour_scale)
    cut = render(frame, S, early_stop=True, stop_schedule=v if kind == "schedule" else None)
    cut.pop("ws")
    return one, cut, eps


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_case(frame, sl, one, cut, eps, terminating=True):
    """assertions 1 - 9 of the module's contract; returns the figures of the case"""
    from dsnerf_amd import _lib
    S, kind, v = sl
    b = SR.bounds_of(S, kind, v)
    K = len(b) - 1
    tr, z, d = one["transparent"], one["z"], one["d"]
    R = tr.shape[0]
    assert np.array_equal(tr, cut["transparent"]) and np.array_equal(bits(z), bits(cut["z"]))
    assert int(one["counts"][CNT_FLAGGED]) == 0 and int(cut["counts"][CNT_FLAGGED]) == 0
    active = int((~tr).sum())
    assert one["stats"]["active"] == cut["stats"]["active"] == active
    res = SR.restate(one["sigma"], tr, z, d, b, eps)
    c = SR.counts(res)
    dead, alive, undet, nt = res["dead"], res["alive"], res["undet"], res["nt"]
    s1, s2 = one["sigma"], cut["sigma"]
    same = (bits(s1) == bits(s2)) | (np.isnan(s1) & np.isnan(s2))
    was_dead = np.zeros(R, bool)
    upto = np.full(R, S, np.int64)                        # the samples in front of a ray's first dead slice
    for k in range(K):
        cols = slice(b[k], b[k + 1])
        A = (same[:, cols] | tr[:, cols]).all(1)          # the one-pass density on every non-transparent sample
        D = (s2[:, cols] == 0).all(1)                     # no density at all
        assert A[alive[:, k]].all(), (k, int((~A & alive[:, k]).sum()), "alive rays without the one-pass density")           # 1
        assert D[dead[:, k]].all(), (k, int((~D & dead[:, k]).sum()), "dead rays with a density")                            # 2
        assert (A | D)[undet[:, k]].all(), (k, "an undetermined ray went both ways inside one slice")                        # 3
        assert D[was_dead].all(), (k, "a ray came back to life")
        now = ~was_dead & (dead[:, k] | (undet[:, k] & D & ~A))
        upto[now] = b[k]
        was_dead |= now
    skipped = cut["stats"]["skipped"]
    assert c["skipped_certain"] <= skipped <= c["skipped_certain"] + c["skipped_undetermined"], (skipped, c)                 # 4
    inside = np.arange(S)[None, :] < upto[:, None]
    assert np.array_equal(bits(one["weights"])[inside], bits(cut["weights"])[inside])                                        # 5
    cull = SR.unshaded(s2, cut["weights"], eps).reshape(R, S)
    assert cut["stats"]["unshaded"] == int(cull.sum()), (cut["stats"], int(cull.sum()))                                      # 6
    assert (cut["colour"][cull] == 0).all()
    Lu = SR.uniform_len(v, S) if kind == "uniform" else 8                                                                    # 7
    assert one["Lu"] == Lu and one["Lh"] == SR.stats_len(Lu, S)
    would, hist, open_rays = SR.stop_stats(s1, tr, z, d, S, Lu, one["Lh"], eps)
    assert would[0] <= one["stats"]["would_skip"] <= would[0] + would[1], (one["stats"], would)
    rest = one["hist"] - hist
    allowed = np.zeros(hist.shape[0], bool)
    for g0, g1, n in open_rays:
        allowed[g0:g1 + 1] = True
    assert (rest >= 0).all() and (rest[~allowed] == 0).all()
    assert np.array_equal(rest.sum(0), sum((n for _, _, n in open_rays), np.zeros(hist.shape[1], np.int64)))
    assert int(one["hist"].sum()) == active
    cap = max(2, 0.001 * c["dead_decisions"])                                                                                # 8
    line = (f"{frame} {SR.slicing_id(sl)}: R {R} active {active} terminated_rays {c['terminated_rays']} dead_decisions {c['dead_decisions']} "
            f"undetermined {c['undetermined']} skipped {skipped} unshaded {cut['stats']['unshaded']} would_skip {one['stats']['would_skip']} "
            f"eps {float(eps):.4g} m ({SR.M_ULP:g} + {SR.M_ARG:g} |arg|) 2^-23, at most {res['m_max']:.3g} where arg < 40")
    print("stop_slices:", line)
    assert c["undetermined"] <= cap, (c, cap)
    if K == 1:                                                                                                               # 9
        assert skipped == 0 and c["dead_decisions"] == 0 and np.array_equal(bits(one["weights"]), bits(cut["weights"]))
    elif terminating:
        assert c["terminated_rays"] >= 10 and skipped > 0, c
        if b[1] <= 0.65 * S:      # (a first border in the last third - [63, 1] - comes behind most of what termination saves)
            assert skipped >= 0.10 * active, (skipped, active)
    return {"line": line, "bounds": b, "skipped": skipped, "unshaded": cut["stats"]["unshaded"]}


def set_slice_env(setenv, delenv, sl):
    if sl[1] == "uniform":
        setenv("DSN_STOP_SLICE", str(sl[2]))
    else:
        delenv("DSN_STOP_SLICE", raising=False)


@pytest.mark.parametrize("sl", SR.SLICINGS, ids=IDS)
@pytest.mark.parametrize("frame", FRAMES)
def test_slices_against_the_restatement(frame, sl, monkeypatch):
    assert os.environ.get("DSN_STOP_ADVANCE", "r")[0] != "l"
    set_slice_env(monkeypatch.setenv, monkeypatch.delenv, sl)
    one, cut, eps = run_case(frame, sl)
    check_case(frame, sl, one, cut, eps)


def list_mode_arrays(cut):
    """what the two advance modes must agree on: sigma, weights, the colour wherever the compositor reads it (sigma > 0; elsewhere the
    array is never written) and the count words"""
    col = np.where((cut["sigma"] > 0)[..., None], cut["colour"], np.float32(0))
    return {"sigma": cut["sigma"], "weights": cut["weights"], "colour": col, "counts": cut["counts"][:256]}


def test_list_mode_is_bit_identical(tmp_path, monkeypatch):
    """DSN_STOP_ADVANCE=list - k_slice_alive<4> / <8> / <0> advancing the rays of their own entries, with the catch-up over slices a ray had
    no entry in - in a fresh child process: sigma, weights, colours and counters equal this process's default mode, on frames with rays
    that have a transparent gap of at least one whole slice"""
    from dsnerf_amd import _lib
    assert os.environ.get("DSN_STOP_ADVANCE", "r")[0] != "l"
    path = str(tmp_path / "list_mode.npz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DSN_STOP_ADVANCE="list",
               PYTHONPATH=os.pathsep.join([root, os.path.join(root, "oracle"), os.path.join(root, "tests")]))
    env.pop("DSN_STOP_SLICE", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=600)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "LIST_MODE_DUMPED" in p.stdout
    got = np.load(path)
    gaps = 0
    for frame in FRAMES:
        for sl in SR.LIST_MODE_SLICINGS:
            set_slice_env(monkeypatch.setenv, monkeypatch.delenv, sl)
            one, cut, eps = run_case(frame, sl)
            want = list_mode_arrays(cut)
            tag = frame + "|" + SR.slicing_id(sl) + "|"
            for k in ("sigma", "weights", "colour"):
                assert np.array_equal(bits(want[k]), bits(got[tag + k])), (tag, k)
            w, g = want["counts"], got[tag + "counts"]
            assert int(w[_lib.CNT_STOP]) == int(g[_lib.CNT_STOP]) and int(w[_lib.CNT_STOP + 1]) == int(g[_lib.CNT_STOP + 1]), tag
            for word in (_lib.CNT_ACTIVE, _lib.CNT_POS, _lib.CNT_LIT, _lib.CNT_SEL, CNT_FLAGGED):
                assert int(w[word]) == int(g[word]), (tag, word)
            assert np.array_equal(w[64:128], g[64:128]), tag      # samples per slice, live samples per slice
            S = sl[0]
            n = SR.gap_rays(one["transparent"], SR.bounds_of(*sl), one["transparent"].shape[0], S)
            print("stop_slices: list mode", tag, "skipped", int(g[_lib.CNT_STOP]), "rays with a transparent gap of a whole slice:", n)
            assert cut["stats"]["skipped"] > 0
            if frame.startswith("synth"):
                assert n > 0, tag
            gaps += n
    assert gaps > 0


def dense_overflowing_state():
    """overflowing_state with the density head scaled by 200 (weights up to 790, below the 1023 the fp16 weight images hold): sigma in the
    thousands, so that some rays DO end on the quarter of their samples that stays in range (measured with 40 x: 13 rays under uniform
    slices of 8, none under [17, 15, 32])"""
    from test_gpu_round2 import overflowing_state
    sd = overflowing_state("nerf.stage1.4")
    for k in ("nerf.density_net.0.weight", "nerf.density_net.0.bias"):
        sd[k] = sd[k] * np.float32(200.0)
    return sd


@pytest.mark.parametrize("sl", [(64, "uniform", 8), (64, "schedule", [17, 15, 32])], ids=["S64-L8", "S64-17_15_32"])
@pytest.mark.parametrize("frame", ["synth_overflow", "synth_overflowdense"])
def test_flagged_densities_never_end_a_ray(frame, sl, monkeypatch):
    """parameters that overflow fp16 (overflowing_state; and the same with a 200 x denser field, so that rays end at all): a flagged
    density is NaN until the fp32 fallback has run and counts as 0 while the slices run, so the sliced frame's transmittance is an
    upper bound.  The flagged positions cannot be told from the one-pass frames - a flagged sample ends up with the exact kernel's
    value, bit for bit, in the split-fp16 frame and in the fp32 frame alike - so two things are built:
      * the DIRECTION the kernels' comment promises, against the one-pass fp32 frame: no ray is dead in the sliced frame at a slice
        where that frame's T_lo calls it alive ("not dead": the slice holds the one-pass split-fp16 frame's densities bit for bit);
      * the sliced frame's own pre-fallback view, exactly: _lib.field_forward on the workspace's canonical points leaves NaN where the
        forward pass flags a sample and the frame's densities, bit for bit, elsewhere.  The restatement fed the one-pass split-fp16
        densities with those positions zeroed decides every slice: alive slices hold the one-pass densities, dead ones none, and the
        `skipped` counter is the restated count."""
    from dsnerf_amd import _lib
    set_slice_env(monkeypatch.setenv, monkeypatch.delenv, sl)
    S, kind, v = sl
    r = setup(frame)[0]
    R = setup(frame)[1].shape[0]
    pk = r.net.packed(r.device)
    pk.set_early_stop_colour_scale(1.0)
    exact = render(frame, S, fp32=True)
    one = render(frame, S, stop_stats=True)
    x_c = workspace_arrays(one["ws"], R * S)["x_c"]
    pk.set_early_stop_colour_scale(max(1.0, _lib.EARLY_STOP_COLOUR_HEADROOM * one["stats"]["colour_max"]))
    eps = SR.eps_scaled(S, pk.colour_scale)
    cut = render(frame, S, early_stop=True, stop_schedule=v if kind == "schedule" else None)
    flagged = int(cut["counts"][CNT_FLAGGED])
    assert flagged > 0 and np.isfinite(cut["sigma"]).all()
    tr = one["transparent"]
    b = SR.bounds_of(S, kind, v)
    K = len(b) - 1
    same = bits(one["sigma"]) == bits(cut["sigma"])
    res = SR.restate(exact["sigma"], tr, one["z"], one["d"], b, eps)
    for k in range(K):
        cols = slice(b[k], b[k + 1])
        A = (same[:, cols] | tr[:, cols]).all(1)
        assert A[res["alive"][:, k]].all(), ("fp32", k, int((~A & res["alive"][:, k]).sum()))
    # the pre-fallback view
    pre = _lib.field_forward(r.scene, pk, x_c)[0].cpu().numpy().reshape(R, S)
    torch.cuda.synchronize()
    nan = np.isnan(pre) & ~tr
    assert int(nan.sum()) > 0
    assert np.array_equal(bits(pre)[~nan & ~tr], bits(one["sigma"])[~nan & ~tr])
    res = SR.restate(np.where(nan, np.float32(0), one["sigma"]), tr, one["z"], one["d"], b, eps)
    c = SR.counts(res)
    for k in range(K):
        cols = slice(b[k], b[k + 1])
        A = (same[:, cols] | tr[:, cols]).all(1)
        D = (cut["sigma"][:, cols] == 0).all(1)
        assert A[res["alive"][:, k]].all() and D[res["dead"][:, k]].all() and (A | D)[res["undet"][:, k]].all(), k
    skipped = cut["stats"]["skipped"]
    assert c["skipped_certain"] <= skipped <= c["skipped_certain"] + c["skipped_undetermined"], (skipped, c)
    assert c["undetermined"] <= max(2, 0.001 * c["dead_decisions"]), c
    evaluated = ~tr & ~np.repeat(res["dead"], np.diff(b), axis=1)
    print("stop_slices: flagged", frame, SR.slicing_id(sl), c, "flagged by the forward pass: all samples", int(nan.sum()), "evaluated ones",
          int((nan & evaluated).sum()), "count word of the sliced frame", flagged, "skipped", skipped)
    if not res["undet"].any():
        assert flagged == int((nan & evaluated).sum())         # the sliced frame flags what it evaluates, and nothing else
    if frame == "synth_overflowdense" and kind == "uniform":
        assert c["terminated_rays"] >= 10 and skipped > 0, c


if __name__ == "__main__":
    # the child of test_list_mode_is_bit_identical: the uniform cases under DSN_STOP_ADVANCE=list, dumped for the parent
    assert os.environ.get("DSN_STOP_ADVANCE") == "list" and len(sys.argv) == 2
    dump = {}
    for frame_ in FRAMES:
        for sl_ in SR.LIST_MODE_SLICINGS:
            os.environ["DSN_STOP_SLICE"] = str(sl_[2])
            _, cut_, _ = run_case(frame_, sl_)
            for k_, a_ in list_mode_arrays(cut_).items():
                dump[frame_ + "|" + SR.slicing_id(sl_) + "|" + k_] = a_
    np.savez(sys.argv[1], **dump)
    print("LIST_MODE_DUMPED", len(dump))
