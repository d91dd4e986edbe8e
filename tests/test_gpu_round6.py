"""Round-6 GPU tests: a lazily built nearest-face level belongs to the call that built it; a lazily set frame rendered in chunks
completes its lists once; geometry that follows the early-stop slices; the training step's re-written small kernels.  All through the
C ABI (ctypes), as everywhere."""
import numpy as np
import pytest
import torch

from helpers import state, workspace_arrays
from test_gpu_round2 import full_frame, renderer_with

pytestmark = pytest.mark.gpu


def _same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))


def _frame_inputs(r, batch):
    o, d = r._dev(batch["ray_o"][0]), r._dev(batch["ray_d"][0])
    return o, d, r._dev(batch["near"][0]), r._dev(batch["far"][0])


# ------------------------------------------------------------------------------------------------------------------------
# lists in state lazy = 2 are the lists of the cells ONE call's samples visited
# ------------------------------------------------------------------------------------------------------------------------
def test_lazily_built_lists_are_not_walked_by_a_later_call_without_the_flag():
    """Rays A rendered WITH DSN_LAZY_LISTS on a lazily set frame leave the level holding the lists of the cells A visits.  Disjoint
    rays B rendered on the same frame WITHOUT the flag (a direct C-API caller; the Python binding always passes it) must not walk
    them - round 5 did, and cells only B visits had empty lists: wrong faces, no error.  Now such a call takes the exhaustive sweep:
    bit-identical to B on a fully built frame, and to DSN_NN_EXHAUSTIVE."""
    from dsnerf_amd import _lib
    canon, faces, batch = full_frame(hw=256)          # halves of 2.1 M samples: the fused cell-major path
    r = renderer_with(state("x_w4"), canon, faces, density_screen=False)
    r.eval()
    S = 64
    o, d, n0, f0 = _frame_inputs(r, batch)
    pk = r.net.packed(r.device)
    xyz, poses = r._dev(batch["xyz"][0]), r._dev(batch["poses"][0])
    R = 256 * 256
    A, B = slice(0, R // 2), slice(R // 2, R)

    def render(sl, **kw):
        return _lib.render_rays(r.scene, pk, _lib.RenderWorkspace(r.device), o[sl].contiguous(), d[sl].contiguous(), n0[sl].clone(),
                                f0[sl].clone(), S, r._t_vals(S), **kw)

    r.scene.set_frame(pk, xyz, poses, 5, False, None, None, None, fine_only=True, lazy=False)
    want_a, want_b = render(A), render(B)
    ex_b = render(B, exhaustive=True)
    assert float(want_b["acc_map"].max()) > 0.05
    r.scene.set_frame(pk, xyz, poses, 5, False, None, None, None, fine_only=True, lazy=True)
    got_a = render(A)                                  # (Scene.lazy is set: the binding passes DSN_LAZY_LISTS -> the level is in state 2)
    r.scene.lazy = False                               # what a C caller that forgets the flag does: same device state, no flag
    got_b = render(B)
    r.scene.lazy = True
    again_a = render(A)                                # with the flag the lists are rebuilt for the rays at hand, whatever was there
    for k in want_a:
        assert _same(want_a[k], got_a[k]), k
        assert _same(want_b[k], got_b[k]), k
        assert _same(ex_b[k], got_b[k]), k
        assert _same(want_a[k], again_a[k]), k


def test_lazily_set_frame_rendered_in_small_chunks_completes_its_lists_once():
    """Below DSN_CELLMAJOR_MIN samples a render call on a lazily set frame completes EVERY cell's lists - decided by the level's
    device header, so only the first chunk pays for it (round 5 rebuilt grid parameters and lists per chunk and
    switched the coarse level off again each time).  Chunks == the frame with full lists; afterwards the level is an ordinary one:
    the fused path with the flag and a stage call answer from it."""
    from dsnerf_amd import _lib
    canon, faces, batch = full_frame(hw=128)
    r = renderer_with(state(), canon, faces, density_screen=False)
    r.eval()
    S = 64
    o, d, n0, f0 = _frame_inputs(r, batch)
    pk = r.net.packed(r.device)
    xyz, poses = r._dev(batch["xyz"][0]), r._dev(batch["poses"][0])
    R = 128 * 128
    chunks = [slice(k, k + 4096) for k in range(0, R, 4096)]      # 262 144 samples per call: not the fused path

    def render(sl):
        return _lib.render_rays(r.scene, pk, _lib.RenderWorkspace(r.device), o[sl].contiguous(), d[sl].contiguous(), n0[sl].clone(),
                                f0[sl].clone(), S, r._t_vals(S))

    def header():
        torch.cuda.synchronize()
        off = r.scene._nn_off[0]                          # the posed mesh's fine level (dsn_nn_header_offsets)
        h = r.scene.buf[off:off + 64].view(torch.int32).cpu().numpy()
        return {"ok": int(h[9]), "total": int(h[10]), "lazy": int(h[13])}

    r.scene.set_frame(pk, xyz, poses, 5, False, None, None, None, fine_only=True, lazy=False)
    want = [render(sl) for sl in chunks]
    full = header()
    assert full["ok"] == 1 and full["lazy"] == 0
    r.scene.set_frame(pk, xyz, poses, 5, False, None, None, None, fine_only=True, lazy=True)
    assert header()["lazy"] == 1
    got0 = render(chunks[0])
    h1 = header()
    assert h1 == full, (h1, full)                        # complete after the first chunk: same entry count as the full build
    got = [got0] + [render(sl) for sl in chunks[1:]]
    assert header() == full
    for a, b in zip(want, got):
        for k in a:
            assert _same(a[k], b[k]), k
    pts, _ = _lib.sample(r.scene, o[:64].contiguous(), d[:64].contiguous(), n0[:64].clone(), f0[:64].clone(), S, r._t_vals(S), None, want_pts=True)
    wl = _lib.warp(r.scene, pts[:64], d[:64], S, want_dir=False)
    r.scene.set_frame(pk, xyz, poses, 5, False, None, None, None, fine_only=True, lazy=False)
    wf = _lib.warp(r.scene, pts[:64], d[:64], S, want_dir=False)
    assert torch.equal(wl["x_c"], wf["x_c"]) and torch.equal(wl["transparent"], wf["transparent"])


# ------------------------------------------------------------------------------------------------------------------------
# the co-residency hazard and the training kernels
# ------------------------------------------------------------------------------------------------------------------------
def test_training_backward_beside_frames_leaves_them_bit_identical():
    """The backward of an 8192 x 64 training step on one stream, the shading and the geometry phases of 12 eval frames (256 x 256 x 64,
    own scene + workspace each) back to back on another: every frame's normals, colours, transparency and canonical points equal the
    frame rendered alone, bit for bit.  Round 6 found k_tangent16 and k_adjoint16 to be aggressors like k_field16 (900 - 2700 differing
    normals per repetition in this very set-up, scripts/dbg/race_train.py); they carry DSN_OWN_SIMD since.  The frames are large
    enough for the kernels to overlap (round 5's lesson: its 96 x 96 test never did) - the test checks that they did."""
    import dsnerf_amd
    from dsnerf_amd import _lib, synth
    from cases import make_cfg
    HW, S, NF = 256, 64, 12
    N = HW * HW * S
    canon, faces, batch = full_frame(hw=HW)
    sd = state("x_w4")
    r = renderer_with(sd, canon, faces, density_screen=False)
    r.eval()
    dev = r.device
    o, d, n0, f0 = _frame_inputs(r, batch)
    xyz, poses = r._dev(batch["xyz"][0]), r._dev(batch["poses"][0])
    pk = r.net.packed(dev)
    tv = r._t_vals(S)
    VF = [(_lib.Scene(torch.from_numpy(canon), torch.from_numpy(faces), dev), _lib.RenderWorkspace(dev)) for _ in range(NF)]
    A, B = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    arrays = lambda ws: workspace_arrays(ws, N)      # noqa: E731  (transparent, x_c, sigma, n_w, colour)

    PH = {"geom": _lib.PHASE_GEOMETRY, "field": _lib.PHASE_FIELD, "shade": _lib.PHASE_SHADE}

    def run(scene, ws, phases, out=None, nf=None):
        nn, ff = nf if nf is not None else (n0.clone(), f0.clone())
        for ph in phases:
            if ph == "set":
                scene.set_frame(pk, xyz, poses, 5, False, None, None, None, fine_only=True)
            else:
                out = _lib.render_rays(scene, pk, ws, o, d, nn, ff, S, tv, phases=PH[ph], out=out)
        return out, (nn, ff)

    run(*VF[0], ["set", "geom", "field", "shade"])
    torch.cuda.synchronize()
    ref = arrays(VF[0][1])
    pos, live = ref["sigma"] > 0, ref["transparent"] == 0
    assert int(pos.sum()) > 100000
    # the aggressor: a training step's backward through the Renderer (forward alone, backward beside the victims)
    Rt = 8192
    sel = np.linspace(0, HW * HW - 1, Rt).astype(np.int64)
    cfg = make_cfg(S)
    net = dsnerf_amd.DualSpaceNeRF(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.to(dev)
    rt = dsnerf_amd.Renderer(net, None, cfg, torch.from_numpy(canon), body_data={"f": faces}, device=dev)
    rt.train()
    tb = {"ray_o": o[sel][None].contiguous(), "ray_d": d[sel][None].contiguous(), "xyz": xyz[None], "poses": poses[None],
          "Th": torch.zeros(1, 1, 3, device=dev), "frame": torch.tensor([5])}
    target = torch.from_numpy(synth.hash_uniform(Rt * 3, 77).reshape(Rt, 3).astype(np.float32)).to(dev)

    def forward():
        torch.manual_seed(3)
        bb = dict(tb)
        bb["near"], bb["far"] = n0[sel][None].clone(), f0[sel][None].clone()
        net.zero_grad()
        return torch.nn.functional.mse_loss(rt.render(bb)["coarse"]["color"], target)

    def both(victims):
        with torch.cuda.stream(A):      # (autograd runs a node's backward on the stream its forward ran on)
            loss = forward()
        torch.cuda.synchronize()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        with torch.cuda.stream(A):
            e[0].record()
            loss.backward()
            e[1].record()
        with torch.cuda.stream(B):
            e[2].record()
            victims()
            e[3].record()
        torch.cuda.synchronize()
        return e[0].elapsed_time(e[1]), e[2].elapsed_time(e[3]), e[0].elapsed_time(e[3])

    overlapped = 0
    for rep in range(2):
        held = [run(sc, ws, ["set", "geom", "field"]) for sc, ws in VF]
        ta, tb_, tall = both(lambda: [run(sc, ws, ["shade"], ob, nfb) for (sc, ws), (ob, nfb) in zip(VF, held)])
        overlapped += int(tall < 0.85 * (ta + tb_))
        for sc, ws in VF:
            a = arrays(ws)
            assert torch.equal(torch.nan_to_num(a["n_w"][pos], nan=-7.0), torch.nan_to_num(ref["n_w"][pos], nan=-7.0))
            assert torch.equal(torch.nan_to_num(a["colour"][pos], nan=-7.0), torch.nan_to_num(ref["colour"][pos], nan=-7.0))
        for sc, ws in VF:
            sc.set_frame(pk, xyz, poses, 5, False, None, None, None, fine_only=True)
        ta, tb_, tall = both(lambda: [run(sc, ws, ["geom"]) for sc, ws in VF])
        overlapped += int(tall < 0.85 * (ta + tb_))
        for sc, ws in VF:
            a = arrays(ws)
            assert torch.equal(a["transparent"], ref["transparent"])
            assert torch.equal(a["x_c"][live], ref["x_c"][live])
    assert overlapped >= 2, "the aggressor and the victims did not run at the same time: the test proves nothing"


# ------------------------------------------------------------------------------------------------------------------------
# training forward: the eval frames' fused geometry (sampler classification + lazily built lists + cell-major search + warp)
# ------------------------------------------------------------------------------------------------------------------------
def test_training_geometry_fused_and_lazy_equals_the_per_lane_walk(monkeypatch):
    """An 8192 x 64 training batch (>= DSN_TRAIN_CELLMAJOR_MIN samples) takes the fused path on a lazily set frame since round 6.  The
    same batch with DSN_NN_UNFUSED (k_warp's per-lane list walk on every cell's lists, as rounds 1-5): forward outputs bit for bit,
    and the gradient tensors that are reproducible from run to run bit for bit as well."""
    import dsnerf_amd
    from dsnerf_amd import synth
    from cases import make_cfg
    R, S, HW = 8192, 64, 512
    canon, faces = synth.make_body()
    xyz = synth.pose_body(canon)
    rays = synth.make_rays(HW, HW, xyz, fit_box=True)
    sel = np.linspace(0, HW * HW - 1, R).astype(np.int64)
    sd = state("x_w4")
    cfg = make_cfg(S)
    dev = torch.device("cuda:0")

    def run(lazy):
        net = dsnerf_amd.DualSpaceNeRF(cfg)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        net.to(dev)
        r = dsnerf_amd.Renderer(net, None, cfg, torch.from_numpy(canon), body_data={"f": faces}, device=dev)
        r.train_lazy_lists = lazy
        r.train()
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        b = {"ray_o": T(rays["ray_o"][sel])[None], "ray_d": T(rays["ray_d"][sel])[None], "near": T(rays["near"][sel])[None],
             "far": T(rays["far"][sel])[None], "xyz": T(xyz)[None], "poses": T(synth.make_poses())[None], "Th": torch.zeros(1, 1, 3),
             "frame": torch.tensor([5])}
        torch.manual_seed(11)
        out = r.render(b)["coarse"]
        assert r.scene.lazy == lazy
        target = T(synth.hash_uniform(R * 3, 77).reshape(R, 3).astype(np.float32)).to(dev)
        torch.nn.functional.mse_loss(out["color"], target).backward()
        torch.cuda.synchronize()
        assert r.range_overflow_count() == 0
        fwd = {k: out[k].detach().clone() for k in ("color", "acc_map", "depth_map", "weights", "z_vals")}
        return fwd, {k: p.grad.detach().clone() for k, p in net.named_parameters()}

    fa, ga = run(True)
    fa2, ga2 = run(True)
    monkeypatch.setenv("DSN_NN_UNFUSED", "1")
    fb, gb = run(False)
    monkeypatch.delenv("DSN_NN_UNFUSED")
    for k in fa:
        assert _same(fa[k], fb[k]), k
    # (the trunk's tensors: fixed-order two-stage reductions - reproducible by construction; an atomically accumulated tensor that
    #  happens to repeat in two runs says nothing about a third)
    stable = [k for k in ga if "stage" in k and torch.equal(ga[k], ga2[k])]
    assert len(stable) >= 12
    for k in stable:
        assert torch.equal(ga[k], gb[k]), k
    for k in ga:
        d = float((ga[k] - gb[k]).norm() / gb[k].norm().clamp_min(1e-30))
        assert d < 1e-4, (k, d)


@pytest.mark.gpu
def test_two_stream_backward_equals_the_one_stream_backward(monkeypatch):
    """dsn_render_rays_grad_ex with an auxiliary stream (default since round 6: the colour head / adjoint chain beside the lighting /
    tangent chain) against the same call on ONE stream (DSN_TRAIN_AUX=0).  Every run starts from a fresh workspace filled with 0xFF
    (DSN_POISON_SCRATCH) so that a kernel launched on the wrong stream cannot pass by reading what an earlier, identical run left
    behind - which is how the adjoint seed on the main stream once went unnoticed.  The tensors with fixed-order reductions: bit for
    bit; the atomically accumulated ones: within their own run-to-run spread."""
    import dsnerf_amd
    from dsnerf_amd import synth
    from cases import make_cfg
    monkeypatch.setenv("DSN_POISON_SCRATCH", "1")
    R, S, HW = 2048, 64, 256
    canon, faces = synth.make_body()
    xyz = synth.pose_body(canon)
    rays = synth.make_rays(HW, HW, xyz, fit_box=True)
    sel = np.linspace(0, HW * HW - 1, R).astype(np.int64)
    sd = state("x_w4")
    cfg = make_cfg(S)
    dev = torch.device("cuda:0")

    def run(aux):
        monkeypatch.setenv("DSN_TRAIN_AUX", aux)
        net = dsnerf_amd.DualSpaceNeRF(cfg)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        net.to(dev)
        r = dsnerf_amd.Renderer(net, None, cfg, torch.from_numpy(canon), body_data={"f": faces}, device=dev)
        r.train()
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        b = {"ray_o": T(rays["ray_o"][sel])[None], "ray_d": T(rays["ray_d"][sel])[None], "near": T(rays["near"][sel])[None],
             "far": T(rays["far"][sel])[None], "xyz": T(xyz)[None], "poses": T(synth.make_poses())[None], "Th": torch.zeros(1, 1, 3),
             "frame": torch.tensor([5])}
        torch.manual_seed(11)
        out = r.render(b)["coarse"]
        target = T(synth.hash_uniform(R * 3, 77).reshape(R, 3).astype(np.float32)).to(dev)
        (torch.nn.functional.mse_loss(out["color"], target) + 0.1 * out["acc_map"].mean()).backward()   # (no synchronize in between)
        g = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
        assert r.range_overflow_count() == 0
        assert (r._grad_ws._aux is not None) == (aux == "1")
        for k in ("color", "acc_map", "depth_map", "weights"):           # (ABI 8: the forward forks too - the far canonical search)
            g["out:" + k] = out[k].detach().clone()
        return g

    one, one2, two, two2 = run("0"), run("0"), run("1"), run("1")
    for k in [k for k in one if k.startswith("out:")]:
        for other in (one2, two, two2):
            assert torch.equal(torch.nan_to_num(one[k], nan=-1.0), torch.nan_to_num(other.pop(k), nan=-1.0)), k
        one.pop(k)
    stable = [k for k in one if "stage" in k and torch.equal(one[k], one2[k])]      # (fixed-order reductions: the trunk)
    assert len(stable) >= 12
    for k in one:
        assert torch.isfinite(two[k]).all(), k
        n = one[k].norm().clamp_min(1e-30)
        spread = max(float((one[k] - one2[k]).norm() / n), float((two[k] - two2[k]).norm() / n))
        d = float((one[k] - two[k]).norm() / n)
        if k in stable:
            assert torch.equal(one[k], two[k]) and torch.equal(two[k], two2[k]), k
        else:
            # (5e-6: the soak's bound for atomically summed tensors, profiles/r06_soak.txt - a one-element tensor's two-run spread can be
            #  1e-7 by chance while the next pair differs by 8e-7: seen once; a kernel on the wrong stream moves these by 1e-2)
            assert d <= 4.0 * spread + 5e-6, (k, d, spread)


# ------------------------------------------------------------------------------------------------------------------------
# session 4: the list build's fill pass places the entries from the membership words the count pass leaves
# ------------------------------------------------------------------------------------------------------------------------
def _fine_level_lists(scene):
    """(offsets, the list's entries as raw int32 [total, 4]) of the posed mesh's fine level, read out of the scene blob"""
    a256 = lambda x: (x + 255) & ~255
    off = scene._nn_off[0]
    hdr = scene.buf[off:off + 64].cpu()
    ncell, ok, total, cap = [int(x) for x in hdr[32:48].view(torch.int32)]
    lazy = int(hdr[52:56].view(torch.int32))
    o_offs = off + 256
    o_list = o_offs + a256(4 * (65536 + 1)) + a256(4 * 65536)
    offs = scene.buf[o_offs:o_offs + 4 * (ncell + 1)].view(torch.int32).cpu()
    ent = scene.buf[o_list:o_list + 16 * total].view(torch.int32).reshape(total, 4).cpu()
    return ncell, ok, lazy, total, offs, ent


def test_list_fill_from_membership_words_equals_the_third_sweep(monkeypatch):
    """k_grid_count leaves one bit per superset entry, k_grid_fill moves the entries those bits name: offsets and lists entry for entry
    as with the fill pass that sweeps the superset again (DSN_NN_NO_MEMBER=1, rounds 1-5) - for the build of every cell (set_frame) and
    for the lazy build of the cells a frame's samples visit (render on a lazily set frame)"""
    from dsnerf_amd import _lib
    canon, faces, batch = full_frame(hw=256)
    r = renderer_with(state("x_w4"), canon, faces, density_screen=False)
    r.eval()
    S = 64
    o, d, n0, f0 = _frame_inputs(r, batch)
    pk = r.net.packed(r.device)
    xyz, poses = r._dev(batch["xyz"][0]), r._dev(batch["poses"][0])

    def lists(lazy):
        r.scene.set_frame(pk, xyz, poses, 5, False, None, None, None, fine_only=True, lazy=lazy)
        out = None
        if lazy:
            out = _lib.render_rays(r.scene, pk, _lib.RenderWorkspace(r.device), o, d, n0.clone(), f0.clone(), S, r._t_vals(S))
        torch.cuda.synchronize()
        return _fine_level_lists(r.scene), out

    for lazy in (False, True):
        (nc_a, ok_a, lz_a, tot_a, offs_a, ent_a), out_a = lists(lazy)
        monkeypatch.setenv("DSN_NN_NO_MEMBER", "1")
        (nc_b, ok_b, lz_b, tot_b, offs_b, ent_b), out_b = lists(lazy)
        monkeypatch.delenv("DSN_NN_NO_MEMBER")
        assert (nc_a, ok_a, lz_a, tot_a) == (nc_b, ok_b, lz_b, tot_b) and tot_a > 100000, (lazy, nc_a, ok_a, lz_a, tot_a, tot_b)
        assert (ok_a == 1) if not lazy else (lz_a == 2)
        assert torch.equal(offs_a, offs_b), lazy
        assert torch.equal(ent_a, ent_b), lazy
        if lazy:
            for k in out_a:
                assert _same(out_a[k], out_b[k]), k
