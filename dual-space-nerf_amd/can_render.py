"""Host-side mirror of the reference's Renderer (the upper drop-in boundary).

Same constructor, attributes and methods as /root/reference/can_render.py:14-406 so that
trainer.py:70 (`render.render(batch)`), test.py:60 / validate.py:50 (`render.render_view(batch)`),
utils/visualizer.py:47-66 (`w2l_without_lbs`, `query_volume`, `.canonical_model`) and
validate.py:27 (`render.net.load_state_dict`) can use it unchanged.  Orchestration is Python; every
number is produced by libdsnerf_hip.so (no torch math, no fallback).

What differs from the reference, on purpose (DESIGN.md "boundary"):
  * a frame is rendered in one pass over ALL its rays (the reference loops over 3072-ray chunks with
    an empty_cache + 6 device->host copies each, can_render.py:172-245); one device->host copy at the end;
  * in eval mode the networks are evaluated only on non-transparent samples (their sigma is zeroed and
    their colour has weight 0 in the reference, can_render.py:115-120) - outputs are identical;
  * `render()` in train mode returns tensors attached to ONE autograd node whose backward is
    dsn_render_rays_grad (analytic parameter gradients, csrc/dsn_train.hip) instead of an op-by-op graph;
  * `render_views(batches)` (not in the reference): the per-frame loop of novel_pose_vis.py:41-66 with several frames in
    flight on their own HIP streams.

Eval-mode safety nets: the plain-fp16 density screen runs with a margin CALIBRATED for the loaded
parameters (first eval frame after the parameters changed: `screen_info`), can be audited on every frame
(`screen_audit = True`, `last_screen_audit()`), and samples whose activations leave the fp16 range of the split-fp16
kernels are re-evaluated in exact fp32 inside the library.  `early_stop` ("auto" | True | False): eval frames front to back
in slices of 4-8 samples with ray termination below a transmittance of eps(S, c) = min(2^-20, 1e-4 / (2 (S + 1) max(1, c)))
(DSN_EARLY_STOP: within (S + 1) eps c = 5e-5 ABSOLUTE of the one-pass frame for colours up to the scale c) - "auto" decides per
parameter version from the statistics of the first eval frame, which also measures the colours (c = 2 x the largest colour that
frame weighed; later frames are watched and raise it), without a wait.  The one default-on feature that is error-bounded instead of
bit-identical: `last_frame_info` says per frame whether it ran and with which threshold.
"""
from __future__ import annotations

import os
import warnings
import weakref

import numpy as np
import torch

from . import _lib


def load_bodydata(model_type="smpl", gender="neutral", model_path=""):
    """utils/smpl_utils.py:3-14: unpickle the SMPL model (dict with 'f', 'weights', 'kintree_table')."""
    import os
    import pickle

    if os.path.isdir(model_path):
        model_path = os.path.join(model_path, "{}_{}.pkl".format(model_type.upper(), gender.upper()))
    assert os.path.exists(model_path), "Path {} does not exist!".format(model_path)
    with open(model_path, "rb") as f:
        return pickle.load(f, encoding="latin1")


_OUT_KEYS = ("color", "disp_map", "acc_map", "depth_map", "weights", "z_vals")
SCREEN_AUDIT_EVERY = 8        # Renderer.screen_audit = "auto": one eval frame in this many carries the density screen's audit


class _HostPoolGuard:
    """Keeps torch's intra-op OpenMP pool from starving the thread that feeds the GPU (VERDICT r02 missing #4).

    The reference's callers run torch CPU ops on the main thread between frames (test.py:61-76: torch.clamp, psnr, .cpu()).
    On the GPU boxes such an op wakes the whole libgomp team - torch.get_num_threads() = 128-256 threads - and every one of
    them then busy-waits at the pool's dock for GOMP_SPINCOUNT iterations (milliseconds) for a next parallel region: a few
    hundred CPU-milliseconds of spinning per op, right while render_view stages its uploads, enqueues the frame and waits for
    it (36 ms per 512 x 512 frame instead of 19, BENCH_r02).  libgomp reads its wait policy once, at load, so it cannot be made
    passive from here; but when a parallel region starts with a SMALLER team, libgomp retires the pool's surplus threads at
    once (gomp_team_start: the dock barrier is re-initialised, threads without a new task leave their loop).  So: cap the
    team at `limit` threads, run one tiny parallel region, render, and put the caller's thread count back - the next big
    torch op of the caller re-creates its team (~10 us per thread).  limit = None / pool already small: nothing happens."""

    _poke = None

    def __init__(self, limit):
        self.limit = limit
        self.saved = None

    def __enter__(self):
        lim = self.limit
        if lim is None or not torch.get_num_threads() > max(2, int(lim)):
            return self
        self.saved = torch.get_num_threads()
        torch.set_num_threads(max(2, int(lim)))
        if _HostPoolGuard._poke is None:
            _HostPoolGuard._poke = torch.zeros(1 << 17)          # > 2 x at::internal::GRAIN_SIZE: goes through at::parallel_for
        _HostPoolGuard._poke.add_(1.0)
        return self

    def __exit__(self, *exc):
        if self.saved is not None:
            torch.set_num_threads(self.saved)
        return False


class _RenderRays(torch.autograd.Function):
    """render_rays as one differentiable node: forward = dsn_render_rays_train, backward = dsn_render_rays_grad
    (what loss.backward() does in trainer.py:70-81).  Inputs that are not parameters carry no gradient, as in the
    reference (rays, near/far, xyz, poses are data).

    The forward leaves its activations in the renderer's ONE shared GradWorkspace; `_cache_gen` says whose they are.  A
    backward whose generation is no longer current recomputes them - into the same workspace, so it takes a new generation
    itself: with several renders outstanding every backward but (at most) the latest recomputes, and none reads another
    call's activations.  The parameters go through save_for_backward, so an in-place update between forward and backward
    (optimizer.step()) raises like it does for an op-by-op graph."""

    @staticmethod
    def forward(ctx, renderer, call, *params):
        o, d, near, far, S, jitter, noise, uniform, frame_args = call
        if not hasattr(renderer, "_grad_ws"):
            renderer._grad_ws = _lib.GradWorkspace(renderer.device)
        renderer._cache_gen = getattr(renderer, "_cache_gen", 0) + 1      # whose activations the cache holds
        out = _lib.render_rays(renderer.scene, renderer.net.packed(renderer.device), renderer._ws, o, d, near, far, S,
                               renderer._t_vals(S), jitter, noise, skip_transparent=False, uniform=uniform,
                               train_cache=renderer._grad_ws)
        ctx.save_for_backward(*params)
        ctx.renderer, ctx.call, ctx.gen = renderer, (o, d, noise, frame_args), renderer._cache_gen
        ctx.frame_key = renderer.scene.frame_key
        ctx.z_vals = out["z_vals"]
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(out["z_vals"])
        return tuple(out[k] for k in _OUT_KEYS)

    @staticmethod
    def backward(ctx, g_color, g_disp, g_acc, g_depth, g_weights, g_z):
        r = ctx.renderer
        o, d, noise, frame_args = ctx.call
        xyz, poses, frame, zero_code, ls, rot, rc = frame_args
        saved = ctx.saved_tensors                           # raises if a parameter was modified in place since the forward
        params = [p.detach() for p in saved]
        sd = dict(zip(_lib.PARAM_ORDER, params))
        packed = r.net.packed(r.device)
        cached = ctx.gen == getattr(r, "_cache_gen", -1)
        # another frame was set since this call's forward - or the activations have to be recomputed and the frame was set lazily
        # (its lists belong to the forward's render call: the recomputation's warp needs every cell's)
        if r.scene.frame_key != ctx.frame_key or (not cached and r.scene.lazy):
            r.scene.set_frame(packed, xyz, poses, frame, zero_code, ls, rot, rc)
            r._frame_src = None
        if g_color is None:
            g_color = torch.zeros(o.shape[0], 3, device=r.device)
        if not hasattr(r, "_grad_ws"):
            r._grad_ws = _lib.GradWorkspace(r.device)
        if not cached:
            r._cache_gen = getattr(r, "_cache_gen", 0) + 1  # the recomputation below overwrites the shared workspace
        grads = _lib.render_rays_grad(r.scene, sd, poses, frame, zero_code, o, d, ctx.z_vals, noise, g_color, g_disp, g_acc,
                                      g_depth, g_weights, ws=r._grad_ws, packed=packed, cached=cached)
        r._note_training_range(_lib.grad_range_word(r._grad_ws, *ctx.z_vals.shape))
        grads = [g.to(device=p.device, dtype=p.dtype).reshape(p.shape) for g, p in zip(grads, saved)]
        return (None, None) + tuple(grads)


class _ViewSlot:
    """scene + workspace + stream of one frame in flight (render_views)"""

    def __init__(self, renderer, own_scene):
        self.scene = renderer.scene if not own_scene else _lib.Scene(renderer.canonical_model["vertex"], renderer.face_idx,
                                                                    renderer.device)
        # (a new slot's workspace starts with the record capacity the renderer's frames were seen to need)
        self.ws = renderer._ws if not own_scene else _lib.RenderWorkspace(renderer.device, fraction=renderer._ws.want_fraction)
        self.stream = torch.cuda.Stream(device=renderer.device)


class _Renderers:
    alive = 0          # Renderer objects of this process (the host-pool fit is undone when the last one is gone)
    lowered = None     # (the caller's torch.get_num_threads(), what fit_host_pool lowered it to)


def hier_retry(attempt, dilate=1, max_dilate=3):
    """The retry rule of extract_mesh(coarse=...): attempt(r) -> (result, info) builds the coarse-to-fine grid with r rings of
    dilation, info["leaks"] being its certificate.  The first attempt runs with `dilate`; while leaks > 0 and r < max_dilate it is
    repeated with one more ring.  Returns (result, info) of the last attempt, info extended by "attempts" and "fell_back"; result is
    None where the last attempt still leaks - the caller then falls back to the dense grid (fell_back = True)."""
    r, attempts = int(dilate), 0
    while True:
        result, info = attempt(r)
        attempts += 1
        if info["leaks"] == 0 or r >= max_dilate:
            break
        r += 1
    fell_back = info["leaks"] > 0
    info = dict(info, attempts=attempts, fell_back=fell_back)
    return (None if fell_back else result), info


class Renderer:
    def __init__(self, net, fine_net=None, cfg=None, canonical_vertex=None, body_data=None, device=None, host_pool="fit"):
        """`body_data` (optional, not in the reference): dict with 'f' [F,3] (and optionally 'weights',
        'kintree_table') used instead of unpickling cfg.DATASETS.SMPL_PATH - the SMPL file is licensed.
        `host_pool` (not in the reference): "fit" (default) caps torch's intra-op thread pool - a PROCESS-GLOBAL setting - at the
        cgroup's CPU quota, once, with a warning when that lowers the caller's setting (why: _lib.fit_host_pool; the GPU boxes show
        256 hardware threads under a 16-core quota and a pool sized from the former gets the process frozen by the kernel's
        bandwidth control); "keep" leaves the caller's pool alone (also: environment DSN_HOST_POOL=keep), and then only the
        per-frame guard (host_pool_limit, restored after every frame) applies."""
        _lib.require_gpu()
        self.net = net
        self.cfg = cfg
        self.fine_net = fine_net
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.canonical_vertex = canonical_vertex
        self._body_data = body_data
        self.load_body_model(gender="neutral", body_model="smpl", model_path=getattr(cfg.DATASETS, "SMPL_PATH", ""))
        self.sample_points_mode = cfg.MODEL.sample_points_mode
        self._ws = _lib.RenderWorkspace(self.device)
        self._tvals = {}
        self._frame_src = None
        self._slots = []
        self.skip_transparent = True      # eval mode: networks only on non-transparent samples (exact)
        # eval frames: the posed mesh's nearest-face lists are built by the frame's own render call, for the cells its samples visit
        # (DSN_FRAME_LAZY_LISTS: same lists entry for entry, for 48 % of the cells on a whole 512 x 512 frame, a tenth on a rank's
        # block of a partitioned frame).  False: every cell's lists in dsn_set_frame, as rounds 1-4 did.
        self.lazy_lists = True
        self.train_lazy_lists = True
        # eval mode: plain-fp16 density screen in front of the accurate pass.  OPT-IN since round 4: its margin is
        # calibrated for the loaded parameters and audited while it runs - frames are bit-identical with it on or off on everything
        # tested - but that is statistical safety, not a proof, and the one converged checkpoint (w4) calibrates it off anyway.
        # density_screen = True: it runs when its calibration says it is safe and pays (-29 % frame time on an untrained fog).
        self.density_screen = False
        # eval mode: re-check 1/128 of the screened-out samples.  True: every frame (read with last_screen_audit()); "auto" (default):
        # the first frame after a calibration and every SCREEN_AUDIT_EVERY-th one after it, read back WITHOUT a wait at the start
        # of a later frame - a violation (a dropped sample whose accurate density is positive) switches the screen off with a
        # warning.  The margin is calibrated on one pose: this is what watches every other pose in production.
        self.screen_audit = "auto"
        self._audit_probe = None          # (count words, event) of an audited frame still to be looked at
        self._audit_frames = 0
        self.screen_info = None           # what the last calibration of the screen found (PackedParams.calibrate_screen)
        # eval mode: front-to-back slices with ray termination (DSN_EARLY_STOP; pixel error <= (S + 1) eps(S, c) x colour = 5e-5 absolute
        # for colours up to the scale c).  "auto": the first eval frame of a parameter version also counts what termination would
        # leave out (DSN_STOP_STATS) and how large its colours are; from the next frame on it is used if it leaves out at least
        # _lib.EARLY_STOP_MIN_SKIPPED of the non-transparent samples, with c = 2 x the largest colour seen (every
        # SCREEN_AUDIT_EVERY-th sliced frame is looked at again, without a wait: larger colours raise c, with a warning).
        # True: the same probe frame, then sliced whatever it leaves out; False switches it off.
        self.early_stop = "auto"
        self._stop_probe = None           # (packed generation, count words, event) of a frame whose statistics are still to be read
        self._guards = []                 # counter copies of the sliced frames enqueued since the last hand-over (_stop_guard)
        self._guard_pool = []             # page-locked 256-byte buffers for them
        self._one_pass_only = False       # set while a frame that broke its early-stop bound is rendered again
        # "auto": the slice lengths of sliced frames follow the probe frame's statistics (longer slices where few rays end: fewer
        # launches, a few more samples, the same error bound - dsn_render_rays_ex); None: uniform slices of 4 / 8 samples
        self.stop_schedule = "auto"
        self._stop_frames = 0
        # render_view / render_views: torch's intra-op pool is capped at this many threads while a frame is staged, enqueued and
        # awaited (_HostPoolGuard; None = leave the pool alone); and for good at the cgroup's CPU quota (_lib.fit_host_pool: a pool
        # larger than the quota gets the whole process frozen by the kernel's bandwidth control whenever the caller runs a torch op)
        self.host_pool_limit = 8
        # train mode: where the stratified jitter and the density noise come from.  "host" (default): the CPU default generator in the
        # reference's order (_draws) - the reference's stream, which pins train-mode outputs to its own.  "device": dsn_train_draws, a
        # pure function of (seed, step, ray id, sample, kind) - not the reference's values, but independent of every other torch.rand
        # call, of the order of the rays and of the rank that holds them, and repeatable from draw_state() alone (seed_draws).
        self.draws = "host"
        self._draw_seed = 0
        self._draw_step = 0
        self.last_draws = None            # (jitter, noise) of the last train-mode render call (tests read them)
        if host_pool not in ("fit", "keep"):
            raise ValueError('host_pool must be "fit" or "keep"')
        self.host_pool = _lib.fit_host_pool(keep=(host_pool == "keep"))
        _Renderers.alive += 1
        if self.host_pool[0] != self.host_pool[1] and _Renderers.lowered is None:
            _Renderers.lowered = (self.host_pool[0], self.host_pool[1])      # (the caller's setting, what it was lowered to)

    def __del__(self):
        # the pool setting is the process's, not this object's: when the LAST Renderer goes away and nobody has
        # changed the setting since it was lowered, the caller gets back the value it had
        try:
            _Renderers.alive -= 1
            if _Renderers.alive == 0 and _Renderers.lowered is not None:
                before, now = _Renderers.lowered
                _Renderers.lowered = None
                if torch.get_num_threads() == now:
                    torch.set_num_threads(before)
        except Exception:
            pass

    # ---- mode switches (reference :26-38) ----
    def train(self):
        self.net.training = True
        self.net.train()
        if self.fine_net is not None:
            self.fine_net.training = True
            self.fine_net.train()

    def eval(self):
        self.net.training = False
        self.net.eval()
        if self.fine_net is not None:
            self.fine_net.training = False
            self.fine_net.eval()

    # ---- body model (reference :382-406) ----
    def load_body_model(self, gender, body_model, model_path):
        tmp = self._body_data if self._body_data is not None else load_bodydata(body_model, gender, model_path)
        if "kintree_table" in tmp:
            parents = torch.as_tensor(np.asarray(tmp["kintree_table"])[0].astype(np.int64)).long()
            parents[0] = -1
            self.parents = parents
        if "weights" in tmp:
            self.smpl_blend_weight = torch.as_tensor(np.asarray(tmp["weights"], np.float32))[None].to(self.device)
        self.face_idx = torch.as_tensor(np.asarray(tmp["f"]).astype(np.int64)).long().to(self.device)
        if self.canonical_vertex is not None:
            cv = torch.as_tensor(self.canonical_vertex, dtype=torch.float32).reshape(-1, 3).to(self.device)
            self.canonical_model = {"vertex": cv, "meshes": cv[self.face_idx]}
            self.scene = _lib.Scene(cv, self.face_idx, self.device)

    # ---- helpers ----
    def _t_vals(self, S):
        # torch.linspace on the host, exactly as utils/pts_utils.py:4 does, then uploaded once
        if S not in self._tvals:
            self._tvals[S] = torch.linspace(0.0, 1.0, steps=S).to(self.device)
        return self._tvals[S]

    def _dev(self, t, dtype=torch.float32):
        """Tensor on the device.  Host tensors of a batch (the reference's DataLoader hands over pageable CPU tensors and calls
        .cuda() on them, can_render.py:100-103,138-141) go through a small ring of persistent page-locked staging buffers and an
        asynchronous copy: a pageable .to(device) of a few MB costs 10-20 ms on the GPU boxes (the runtime pins and unpins the
        pages and waits for the stream), 70 ms per 512 x 512 batch (scripts/render_view_probe.py)."""
        if t.is_cuda or t.numel() * t.element_size() < (1 << 16) or t.is_pinned() or self.device.type != "cuda":
            return t.to(device=self.device, dtype=dtype).contiguous()
        n = t.numel()
        ring = getattr(self, "_stage_ring", None)
        if ring is None:
            ring = self._stage_ring = {"i": 0, "slots": [{"host": None, "done": torch.cuda.Event()} for _ in range(8)]}
        slot = ring["slots"][ring["i"]]
        ring["i"] = (ring["i"] + 1) % len(ring["slots"])
        slot["done"].synchronize()                       # the copy that last read this staging buffer has finished
        nbytes = n * dtype.itemsize
        if slot["host"] is None or slot["host"].numel() < nbytes:
            slot["host"] = torch.empty(max(nbytes, 1 << 22), dtype=torch.uint8).pin_memory()
        stage = slot["host"][:nbytes].view(dtype).view(t.shape)
        # host memcpy (with the dtype conversion, if any) through numpy: ONE thread.  torch's copy_ fans a few MB out over its
        # whole intra-op pool - 128-256 threads on the GPU boxes - whose threads then spin beside the thread that feeds the GPU:
        # a 1 MB torch CPU op in front of a frame costs the frame 7-14 ms (scripts/h2h_caller_probe.py)
        if t.device.type == "cpu" and not t.requires_grad and t.dtype != torch.bfloat16:
            np.copyto(stage.numpy(), t.numpy(), casting="unsafe")
        else:
            stage.copy_(t)
        out = torch.empty(t.shape, dtype=dtype, device=self.device)
        out.copy_(stage, non_blocking=True)
        slot["done"].record()
        return out

    # Which tensor the scene's posed mesh came from.  Identity, not address: a DataLoader hands a NEW tensor per batch that
    # routinely reuses the freed address of the previous one, and an in-place update keeps the address - so the
    # key is a weak reference to the tensor object plus its version counter.
    def _mark_frame_src(self, xyz):
        self._frame_src = (weakref.ref(xyz), xyz._version)

    def _is_frame_src(self, xyz):
        src = self._frame_src
        return src is not None and src[0]() is xyz and src[1] == xyz._version

    def _set_frame(self, batch, scene=None, frame=None, lazy=False):
        """dsn_set_frame from a batch.  Returns the arguments as used (device tensors), which a training forward keeps for
        its backward.  lazy: the frame is about to be rendered by _lib.render_rays (eval frames): only the posed mesh's fine grid is
        laid out here and the render call builds the candidate lists of the cells its samples visit (DSN_FRAME_LAZY_LISTS)."""
        scene = self.scene if scene is None else scene
        if frame is None:
            frame = int(torch.as_tensor(batch["frame"]).reshape(-1)[0])
        zero_code, ls, rot, rc = self.net.frame_args(batch)
        xyz = self._dev(batch["xyz"][0])
        poses = batch["poses"][0].to(device=self.device, dtype=torch.float32).contiguous()
        # (fine level only: the samples of rays clipped to the body's bounds never leave it; stage calls on far-away points - w2l
        #  on arbitrary points - still get the exact index, from the exhaustive sweep)
        scene.set_frame(self.net.packed(self.device), xyz, poses, frame, zero_code, ls, rot, rc, fine_only=True,
                        lazy=bool(lazy) and self.lazy_lists)
        if scene is self.scene:
            self._mark_frame_src(batch["xyz"])
        return (xyz, poses, frame, zero_code, ls, rot, rc)

    def _screen_usable(self, frame=None):
        """eval mode: is the density screen on for this frame?  Calibrates its margin for the current parameters first
        (once per parameter version: synchronises then).  Needs the scene's frame state to be set.  frame = (scene, workspace, R, S)
        of a frame whose geometry phase has run: the calibration then uses that frame's own canonical points (what _render_eval
        does on the first eval frame of a parameter version); without it, a cube around the canonical centroids."""
        if not (self.density_screen and self.skip_transparent):
            return False
        packed = self.net.packed(self.device)
        if packed.screen is None:
            info = packed.calibrate_screen(self.scene) if frame is None else packed.calibrate_screen(frame[0], frame=frame[1:])
            self.screen_info = dict(info)
            if not info["safe"]:
                warnings.warn("dsnerf_amd: the plain-fp16 density screen would need a margin of %.3g of the term magnitude for these "
                              "parameters (cap %.3g; largest deviation %.3g): it stays off, every non-transparent sample takes the "
                              "accurate pass" % (_lib.SCREEN_HEADROOM * info["margin_statistic"], _lib.SCREEN_MARGIN_CAP,
                                                 info["deviation"]))
        return packed.screen_pays(self._early_stop_in_use(packed))

    def _early_stop_in_use(self, packed):
        if self.early_stop == "auto":
            return bool(packed.early_stop and packed.early_stop["usable"])
        return bool(self.early_stop)

    def _draws(self, R, S):
        """Train-mode random draws from the CPU default generator in the reference's order:
        torch.rand([1,R,S]) (utils/pts_utils.py:12) then torch.randn([R,S]) (utils/nerf_net_utils.py:31)."""
        want_j = self.net.training and self.cfg.MODEL.perturb > 0.0
        want_n = self.net.training and self.cfg.MODEL.raw_noise_std > 0.0
        if not (want_j or want_n):
            return None, None
        if self.device.type != "cuda":
            raise RuntimeError("dsnerf_amd renders on the GPU only")
        # The draws go straight into a small ring of persistent page-locked staging buffers (out=: same generator
        # stream as a fresh tensor) and are uploaded with one asynchronous copy.  Fresh 2 MB host tensors cost 10-80 ms
        # per step on the GPU boxes (page faults of newly mapped memory + the runtime pinning them for the pageable
        # copy, which also blocks until the stream has drained): scripts/train_host_probe.py.
        n = 2 * R * S
        ring = getattr(self, "_draw_ring", None)
        if ring is None or ring["n"] < n:
            ring = self._draw_ring = {"n": n, "i": 0, "slots": [
                {"host": torch.empty(n, dtype=torch.float32).pin_memory(), "dev": torch.empty(n, device=self.device),
                 "done": torch.cuda.Event()} for _ in range(3)]}
        slot = ring["slots"][ring["i"]]
        ring["i"] = (ring["i"] + 1) % len(ring["slots"])
        slot["done"].synchronize()            # the copy that last read this staging buffer (three draws ago) has finished
        k = 0
        if want_j:
            torch.rand(1, R, S, out=slot["host"][:R * S].view(1, R, S))
            k = R * S
        m = k
        if want_n:
            hn = slot["host"][k:k + R * S].view(R, S)
            torch.randn(R, S, out=hn)
            if float(self.cfg.MODEL.raw_noise_std) != 1.0:
                hn.mul_(self.cfg.MODEL.raw_noise_std)
            m = k + R * S
        slot["dev"][:m].copy_(slot["host"][:m], non_blocking=True)
        slot["done"].record()
        # device-side clones (two 5 us copies): autograd may keep the draws alive for longer than the ring does
        jitter = slot["dev"][:R * S].view(R, S).clone() if want_j else None
        noise = slot["dev"][k:k + R * S].view(R, S).clone() if want_n else None
        return jitter, noise

    # ---- draws="device": the same two arrays from dsn_train_draws (the rule of include/dsnerf.h) ----
    def seed_draws(self, seed, step=0):
        """seed (taken modulo 2^64) and step counter (modulo 2^32) of the device draws: every train-mode render call with
        draws == "device" draws at the current step and then advances it by one"""
        self._draw_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._draw_step = int(step) & 0xFFFFFFFF
        return self

    def draw_state(self):
        """what a checkpoint keeps of the device draws: the next train-mode render call draws at this step"""
        return {"seed": self._draw_seed, "step": self._draw_step}

    def load_draw_state(self, d):
        return self.seed_draws(d["seed"], d["step"])

    def _draw_source(self):
        if self.draws not in ("host", "device"):
            raise ValueError('Renderer.draws must be "host" or "device"')
        return self.draws

    def _device_draws(self, R, S, batch=None, want_jitter=True, want_noise=True):
        """_draws' two arrays at the current step, without advancing it.  The rays' ids: batch["ray_ids"] ([1, R] or [R], int32 or
        int64, on the device - e.g. coord[:, 0] * W + coord[:, 1] of sample_batch), else batch["ray_base"] + r (an int - e.g. a
        rank's offset), else r.  One launch: no pinned memory, no copy from the host, nothing read back."""
        want_j = want_jitter and self.net.training and self.cfg.MODEL.perturb > 0.0
        want_n = want_noise and self.net.training and self.cfg.MODEL.raw_noise_std > 0.0
        if not (want_j or want_n):
            return None, None
        ids, base = None, 0
        if batch is not None and batch.get("ray_ids") is not None:
            ids = batch["ray_ids"]
            if not (torch.is_tensor(ids) and ids.is_cuda and ids.dtype in (torch.int32, torch.int64) and ids.numel() == R):
                raise ValueError("batch['ray_ids'] must be an int32 or int64 device tensor with one id per ray")
            ids = ids.reshape(R).to(torch.int32).contiguous()          # (int64 ids: modulo 2^32, as the rule takes them)
        elif batch is not None and batch.get("ray_base") is not None:
            base = int(batch["ray_base"])
        return _lib.train_draws(R, S, self._draw_seed, self._draw_step, ray_base=base, ray_ids=ids,
                                noise_std=float(self.cfg.MODEL.raw_noise_std), want_jitter=want_j, want_noise=want_n, device=self.device)

    # ---- sampling (reference :40-63) ----
    def get_sampling_points(self, ray_o, ray_d, near, far, xyz, mode="GG"):
        """ray_o/ray_d [1,R,3], near/far [1,R] (updated in place in GG mode), xyz [1,V,3] ->
        pts [1,R,S,3], z_vals [1,R,S].  Needs the frame's xyz in the scene: Renderer.render does that;
        direct callers get it set here from `xyz` with the current pose state untouched."""
        S = self.cfg.MODEL.COARSE_RAY_SAMPLING
        R = ray_o.shape[1]
        o, d = self._dev(ray_o[0]), self._dev(ray_d[0])
        n_dev, f_dev = self._dev(near[0]), self._dev(far[0])
        jitter = None
        if self._draw_source() == "device":      # the rule's jitter at the current step (render() advances it, this does not)
            jitter = self._device_draws(R, S, want_noise=False)[0]
        elif self.net.training and self.cfg.MODEL.perturb > 0.0:
            jitter = torch.rand(1, R, S).reshape(R, S).to(self.device)
        if not self._is_frame_src(xyz):
            self._upload_xyz(xyz)
        pts, z = _lib.sample(self.scene, o, d, n_dev, f_dev, S, self._t_vals(S), jitter, want_pts=True, gg=(mode == "GG"))
        if mode == "GG":   # in-place update like the reference (:52-53)
            near[0].copy_(n_dev.to(near.device))
            far[0].copy_(f_dev.to(far.device))
        return pts[None], z[None]

    def _upload_xyz(self, xyz):
        # posed mesh only (callers without a full batch: the pose code is zeroed until _set_frame runs)
        x = self._dev(xyz.reshape(-1, 3))
        poses = torch.zeros(24, 3, device=self.device)
        self.scene.set_frame(self.net.packed(self.device), x, poses, 0, True, None, None, None)
        self._mark_frame_src(xyz)

    def _ensure_mesh(self, batch):
        """the scene must hold batch['xyz'] as its posed mesh (direct callers of the warp / network stages)"""
        xyz = batch["xyz"]
        if self._is_frame_src(xyz) and not self.scene.lazy:      # (a lazily set frame holds lists for its own render call only)
            return
        if "poses" in batch and "frame" in batch:
            self._set_frame(batch)
        else:
            self._upload_xyz(xyz)

    # ---- warp (reference :299-379) ----
    def w2l(self, pts_world, ray_o_W, ray_d_W, batch):
        B, ray, sp, _ = pts_world.shape
        pts_smpl_can, transparent_mask, ray_d_can = self.w2l_without_lbs(
            pts_world, batch, self.canonical_model, ray_d_W=ray_d_W.unsqueeze(2).expand([-1, -1, sp, -1]).reshape(B, -1, 3))
        d = self._dev(ray_d_W.reshape(-1, 3))
        rays = torch.cat([d[:, None, :].expand(-1, sp, -1).reshape(-1, 3), ray_d_can], dim=-1).reshape(B * ray, sp, 6)
        pw = self._dev(pts_world.reshape(B * ray, sp, 3))
        return torch.cat([pw, pts_smpl_can.reshape(-1, sp, 3)], dim=-1), rays, transparent_mask

    def w2l_without_lbs(self, pts_world, batch, canonical_model, ray_d_W=None, floor=-4, ceil=5):
        """pts_world [B,R,S,3] -> (pts_smpl_can [N,3], transparent_mask [B,N] bool[, ray_d_can [N,3]]).
        ray_d_W, when given, is the per-POINT direction tensor [B,N,3] the reference passes."""
        assert floor == -4 and ceil == 5, "the uv clamp range is compiled in (utils/render_utils.py:103)"
        B, ray, sp, _ = pts_world.shape
        self._ensure_mesh(batch)
        pts = self._dev(pts_world.reshape(-1, 3))
        if ray_d_W is not None:
            d = self._dev(ray_d_W.reshape(-1, 3))   # per point -> S=1 addressing
            out = _lib.warp(self.scene, pts, d, 1, want_dir=True)
            return out["x_c"], out["transparent"].bool().reshape(B, -1), out["ray_d_can"]
        out = _lib.warp(self.scene, pts, None, 1, want_dir=False)
        return out["x_c"], out["transparent"].bool().reshape(B, -1)

    # ---- network + compositing on explicit points (reference :65-134) ----
    def _module_info(self, batch_info, frame_idx):
        """batch_info for a call into self.net with this renderer's scene holding the frame (so the module does not build a
        second scene): reference batch_info needs poses, xyz, Th, canonical_model, face_idx (model/spacenet.py:210-266)."""
        bi = dict(batch_info)
        if "xyz" in bi and "poses" in bi:
            if not self._is_frame_src(bi["xyz"]) or self.scene.frame_key is None:
                fi = int(torch.as_tensor(frame_idx).reshape(-1)[0])
                self._set_frame(bi, frame=fi)
            bi["_dsn_scene"] = self.scene
        return bi

    def render_rays(self, pts, rays, z_vals, frame_idx, net, transparent_mask=None, batch_info=None):
        """can_render.py:97-134.  Differentiable w.r.t. the parameters in train mode (DualSpaceNeRF.forward's autograd node
        + torch ops on its outputs would be the reference's graph; here compositing is dsn_composite, which carries no
        graph - train through Renderer.render, whose single node covers the whole path)."""
        if self.net.training and torch.is_grad_enabled() and any(p.requires_grad for p in self.net.parameters()):
            raise RuntimeError("Renderer.render_rays / batchify_pts build no autograd graph in dsnerf_amd (compositing is one HIP "
                               "kernel): train through Renderer.render, or call them under torch.no_grad() / in eval mode")
        pts, rays, z_vals = self._dev(pts), self._dev(rays), self._dev(z_vals)
        rays_d = rays[:, 0, :3].contiguous()
        B, sp = pts.shape[:2]
        noise = None
        if self._draw_source() == "device":      # the rule's noise at the current step, not advanced (as get_sampling_points' jitter)
            noise = self._device_draws(B, sp, batch_info, want_jitter=False)[1]
        elif self.net.training and self.cfg.MODEL.raw_noise_std > 0.0:
            noise = (torch.randn(B, sp) * self.cfg.MODEL.raw_noise_std).to(self.device)
        bi = self._module_info(batch_info or {}, frame_idx)
        with torch.no_grad():
            rgbs, density, _ = net(pts.reshape(-1, 6), rays.reshape(-1, 6), frame_idx, batch_info=bi)
        tm = None if transparent_mask is None else transparent_mask.to(self.device).reshape(B, sp).to(torch.uint8).contiguous()
        rgb_map, disp_map, acc_map, weights, depth_map = _lib.composite(
            rgbs.reshape(B, sp, 3).contiguous(), density.reshape(B, sp).contiguous(), tm, z_vals, rays_d, noise)
        return {"color": rgb_map, "disp_map": disp_map, "acc_map": acc_map, "depth_map": depth_map,
                "weights": weights, "z_vals": z_vals}

    def batchify_pts(self, pts, rays, z_vals, frame_idx, chunk=1024 * 32, net=None, batch_info=None):
        net = self.net if net is None else net
        return self.render_rays(pts, rays, z_vals, frame_idx, net=net,
                                transparent_mask=batch_info["transparent_mask"], batch_info=batch_info)

    # ---- the datasets' ray sampler (utils/rays_utils.py:104-172, utils/h36m_utils.py:78-146) on the device ----
    def sample_batch(self, img, K, R, T, bounds, mask, nrays, seed, convention="zju", mask_b=None, occupancy_from=None,
                     bound_mask=None, check=True):
        """A training batch drawn on the device (_lib.train_rays, the rule of include/dsnerf.h) from an image, its masks and the
        camera: what the datasets' my_sample_ray (convention "zju", mask = msk_cihp) / sample_ray_h36m ("h36m", mask = msk,
        mask_b = msk_cihp) call builds on the host.  img [H,W,3] float64 or float32; mask, mask_b, occupancy_from (the map
        `occupancy` is gathered from: msk_fg; omitted -> no "occupancy" key) and bound_mask (a box mask of the caller's, e.g. cv2's;
        omitted -> computed) [H,W]; device tensors are used as they are.  The same arguments give the same batch, bit for bit.
        Returns the datasets' keys on the device with the loader's leading 1 - rgb, ray_o, ray_d [1,n,3], near, far [1,n], coord
        [1,n,2] int64, mask_at_box [1,n] bool, occupancy [1,n] uint8, mybound_mask [1,H,W] uint8 - plus "rounds"; render() takes it
        once xyz, poses and frame are added.  check=True reads the status word (one synchronisation): ValueError for an empty body
        or random class or an unusable camera (the reference: ValueError from np.random.randint), RuntimeError for a batch still
        short after _lib.TRAIN_RAYS_MAX_ROUNDS rounds (the reference loops for ever).  check=False leaves the device status word
        in the dict ("status") for the caller to read when it likes."""
        b = _lib.train_rays(img if isinstance(img, torch.Tensor) else torch.as_tensor(img), K, R, T, bounds, mask, nrays, seed,
                            convention=convention, mask_b=mask_b, occupancy_src=occupancy_from, bound_mask_in=bound_mask,
                            workspace=getattr(self, "_sample_ws", None))
        self._sample_ws = b.pop("workspace")
        status = b.pop("status")
        batch = {k: b[k][None] for k in ("rgb", "ray_o", "ray_d", "near", "far", "coord", "mask_at_box")}
        if b["occupancy"] is not None:
            batch["occupancy"] = b["occupancy"][None]
        batch["mybound_mask"] = b["bound_mask"][None]
        batch["rounds"] = b["rounds"]
        if not check:
            batch["status"] = status
            return batch
        s = int(status)
        if s == _lib.TRAIN_RAYS_EMPTY_CLASS:
            raise ValueError("sample_batch: the body class or the box mask is empty (np.random.randint: low >= high)")
        if s == _lib.TRAIN_RAYS_BAD_CAMERA:
            raise ValueError("sample_batch: a corner of the bounds lies behind the camera or projects to nothing finite")
        if s == _lib.TRAIN_RAYS_SHORT:
            raise RuntimeError(f"sample_batch: fewer than {int(nrays)} rays passed the box test in {_lib.TRAIN_RAYS_MAX_ROUNDS} rounds")
        return batch

    # ---- the trainer's call (reference :137-168) ----
    def render(self, batch):
        o, d = self._dev(batch["ray_o"][0]), self._dev(batch["ray_d"][0])
        near, far = self._dev(batch["near"][0]), self._dev(batch["far"][0])
        R = o.shape[0]
        S = self.cfg.MODEL.COARSE_RAY_SAMPLING
        self._poll_training_range()
        sd = dict(self.net.named_parameters())
        differentiable = self.net.training and torch.is_grad_enabled() and any(p.requires_grad for p in sd.values())
        # (lazily set for training too since round 6: the training forward builds the lists of the cells its batch visits, or - small
        #  batches - completes every cell's lists itself; `train_lazy_lists = False` keeps the per-step build of every cell in set_frame)
        frame_args = self._set_frame(batch, lazy=(not differentiable) or self.train_lazy_lists)
        if self._draw_source() == "device" and self.net.training:
            jitter, noise = self._device_draws(R, S, batch)
            self._draw_step = (self._draw_step + 1) & 0xFFFFFFFF
        else:
            jitter, noise = self._draws(R, S)
        if self.net.training:
            self.last_draws = (jitter, noise)
        if self.sample_points_mode not in ("GG", "uniform"):
            raise Exception("error")   # the reference fails on unknown modes too (get_sampling_points returns nothing)
        uniform = self.sample_points_mode == "uniform"
        if differentiable:
            outs = _RenderRays.apply(self, (o, d, near, far, S, jitter, noise, uniform, frame_args),
                                     *[sd[k] for k in _lib.PARAM_ORDER])
            out = dict(zip(_OUT_KEYS, outs))
        else:
            out = self._render_eval(self.scene, self._ws, o, d, near, far, S, jitter, noise)
            out = self._hand_over(out, lambda: self._render_eval(self.scene, self._ws, o, d, near, far, S, jitter, noise))
        if batch["near"].is_cuda:   # in-place semantics of the reference when the batch already lives on the device
            batch["near"][0].copy_(near)
            batch["far"][0].copy_(far)
        batch["canonical_model"] = self.canonical_model
        batch["face_idx"] = self.face_idx
        return {"coarse": out}

    def _eval_plan(self, noise, screen=None):
        """per-frame decisions of an eval-mode frame (needs the scene's frame state for a first calibration): keyword arguments
        of _lib.render_rays"""
        skip = self.skip_transparent and not self.net.training
        if skip and noise is None and self.early_stop in ("auto", True):
            self._read_stop_probe()      # (first: whether the screen pays depends on it)
        if screen is None:
            screen = skip and noise is None and self._screen_usable()
        packed = self.net.packed(self.device)
        stop, stats = False, False
        if skip and noise is None and not self._one_pass_only:
            if self.early_stop in ("auto", True):
                # the first eval frame of a parameter version is rendered in one pass and measures: what termination would leave out,
                # how large the colours are (-> the threshold's colour scale), the slice schedule.  "auto" then slices when it pays;
                # True slices whenever the colours are finite (round 5: it used to slice from the first frame on with the scale 1, which
                # the hand-over check now refuses for any checkpoint whose colours exceed 1)
                if packed.early_stop is None:
                    if self._stop_probe is None:
                        stats = True
                else:
                    stop = packed.early_stop["usable"] if self.early_stop == "auto" else packed.early_stop.get("finite", True)
            else:
                stop = bool(self.early_stop)
        audit = False
        if screen:
            self._read_audit_probe()
            screen = screen and self.density_screen        # (a violation found just now has switched it off)
            if self.screen_audit == "auto":
                audit = self._audit_probe is None and self._audit_frames % SCREEN_AUDIT_EVERY == 0
                self._audit_frames += 1
            else:
                audit = bool(self.screen_audit)
        sched = packed.early_stop.get("schedule") if (stop and packed.early_stop and self.stop_schedule == "auto") else None
        if sched is not None and sum(sched) != int(self.cfg.MODEL.COARSE_RAY_SAMPLING):
            sched = None
        return {"skip_transparent": skip, "uniform": (self.sample_points_mode == "uniform"), "screen": screen,
                "audit": audit, "early_stop": stop, "stop_stats": stats, "stop_schedule": sched}

    def _render_eval(self, scene, ws, o, d, near, far, S, jitter, noise, screen=None, plan=None, phases=0, out=None, lights=None,
                     maps=None):
        """lights: [K, 12] light records (_lib.light_records) - the frame is a relighting sweep (_lib.render_rays_lights; one call, no
        phases), its "color" is [K, R, 3]; maps: names of decomposition maps - the sweep also composites those (_lib.render_rays_maps)"""
        packed = self.net.packed(self.device)
        if (plan is None and screen is None and phases == 0 and noise is None and packed.screen is None and self.density_screen
                and self.skip_transparent and not self.net.training):
            # First eval frame of a parameter version: its geometry phase first (sampler, warp: the canonical points of its
            # non-transparent samples), the density screen's margin calibrated on THOSE points, then the rest of the frame.
            geo = {"skip_transparent": True, "uniform": (self.sample_points_mode == "uniform"), "screen": True, "audit": False,
                   "early_stop": False, "stop_stats": False, "stop_schedule": None}
            out = _lib.render_rays(scene, packed, ws, o, d, near, far, S, self._t_vals(S), jitter, noise, phases=_lib.PHASE_GEOMETRY,
                                   out=out, **geo)
            self._screen_usable(frame=(scene, ws, o.shape[0], S))
            phases = _lib.PHASE_FIELD | _lib.PHASE_SHADE
            if lights is not None:
                out = None      # (a sweep runs whole: its geometry phase again behind the calibration)
        plan = self._eval_plan(noise, screen) if plan is None else plan
        # what this frame ran with (early stop is the one default-on feature whose output is error-bounded, not
        # bit-identical - a caller can see per frame whether it was in use and with which threshold)
        cs = packed.colour_scale
        self.last_frame_info = {"density_screen": bool(plan["screen"]), "screen_audit": bool(plan["audit"]),
                                "early_stop": bool(plan["early_stop"]), "early_stop_schedule": plan.get("stop_schedule"),
                                "early_stop_eps": _lib.early_stop_eps(S, cs) if plan["early_stop"] else None,
                                "early_stop_colour_scale": cs if plan["early_stop"] else None,
                                "early_stop_bound_x_max_colour": (S + 1) * _lib.early_stop_eps(S, cs) if plan["early_stop"] else 0.0,
                                # (absolute, for colours up to the scale)
                                "early_stop_bound_abs": (S + 1) * _lib.early_stop_eps(S, cs) * cs if plan["early_stop"] else 0.0}
        if lights is not None:
            self.last_frame_info["lights"] = int(lights.shape[0])
            if maps is not None:
                out = _lib.render_rays_maps(scene, packed, ws, o, d, near, far, S, self._t_vals(S), lights, maps=maps, **plan)
            else:
                out = _lib.render_rays_lights(scene, packed, ws, o, d, near, far, S, self._t_vals(S), lights, **plan)
        else:
            out = _lib.render_rays(scene, packed, ws, o, d, near, far, S, self._t_vals(S), jitter, noise, phases=phases, out=out,
                                   share_cus=getattr(self, "_frames_overlap", False), **plan)
        if plan["stop_stats"] and (phases == 0 or phases & _lib.PHASE_SHADE):
            self._probe_samples = int(o.shape[0]) * int(S)
            self._probe_shape = (int(o.shape[0]), int(S))
            snap = ws.buf[:_lib.CNT_BYTES].clone()      # (stream-ordered: the next frame on this workspace clears the words)
            ev = torch.cuda.Event()
            ev.record()
            self._stop_probe = (packed.generation, snap, ev)
        if plan["early_stop"] and (phases == 0 or phases & _lib.PHASE_SHADE):
            # EVERY sliced frame leaves its counters for the caller's hand-over point (_stop_guard_ok): the bound of early stop holds for
            # colours up to the scale its threshold was computed with - a frame that weighed a larger colour is rendered again in one
            # pass BEFORE it is handed to the caller (round 4 looked at every 8th frame and only raised the scale for
            # later ones)
            self._guards.append(self._stop_guard(ws, cs, int(o.shape[0]) * int(S)))
            while len(self._guards) > 64:      # (a caller of batchify_rays_view / render_rays that never reaches a hand-over point)
                self._guard_pool.append(self._guards.pop(0)[0])
            self._stop_frames += 1
        if plan["audit"] and self.screen_audit == "auto" and (phases == 0 or phases & _lib.PHASE_SHADE):
            snap = ws.buf[:256].clone()
            ev = torch.cuda.Event()
            ev.record()
            self._audit_probe = (snap, ev)
        return out

    def _read_audit_probe(self, wait=False):
        """screen_audit = "auto": look at the counters of an audited frame once it has finished (no wait unless asked)"""
        if self._audit_probe is None:
            return None
        snap, ev = self._audit_probe
        if not wait and not ev.query():
            return None
        ev.synchronize()
        self._audit_probe = None
        return self._judge_audit(snap.view(torch.int32).cpu())

    def _judge_audit(self, c):
        # (word + 6: the audited samples the judging kernel went through - the raw counter at + 0 runs on past the list's capacity)
        res = {"audited": int(c[_lib.CNT_AUDIT + 6]), "violations": int(c[_lib.CNT_AUDIT + 4]),
               "max_sigma": float(c[_lib.CNT_AUDIT + 5:_lib.CNT_AUDIT + 6].view(torch.float32)[0])}
        self.last_audit = res
        if res["violations"] > 0 and self.density_screen:
            self.density_screen = False
            warnings.warn("dsnerf_amd: the density screen dropped samples with positive density (%d of %d audited, max sigma %.3g): "
                          "screen switched off" % (res["violations"], res["audited"], res["max_sigma"]))
        return res

    def _read_stop_probe(self, wait=False):
        """early_stop = "auto": pick up the statistics of the probe frame once it has finished (no wait unless asked)."""
        if self._stop_probe is None:
            return
        gen, snap, ev = self._stop_probe
        if not wait and not ev.query():
            return
        ev.synchronize()
        self._stop_probe = None
        packed = self.net.packed(self.device)
        if packed.generation != gen:
            return
        st = _lib.read_stop_stats(snap)
        frac = st["would_skip"] / max(st["active"], 1)
        # (the probe frame also says how many relu records frames of these parameters need: a dense field gets a larger record array
        #  before its second frame instead of the overflow pass on every frame)
        n_pos = int(snap.view(torch.int32)[_lib.CNT_POS])
        if getattr(self, "_probe_samples", 0) > 0:
            # (the probe frame is one pass; with termination in use the sliced frames list far fewer samples: estimated by what it leaves
            #  out, corrected by the sliced frames themselves at their hand-over (_stop_guards_ok), covered by the exact overflow pass in between)
            will_stop = frac >= _lib.EARLY_STOP_MIN_SKIPPED if self.early_stop == "auto" else bool(self.early_stop)
            self._fit_records(n_pos / float(self._probe_samples) * ((1.0 - frac) if will_stop else 1.0), 1.6 if will_stop else 1.25)
        self._note_colour_max(packed, st["colour_max"], first=True)
        cm = st["colour_max"]
        finite = cm == cm and cm != float("inf")
        packed.early_stop = {"skipped_fraction": frac, "usable": finite and frac >= _lib.EARLY_STOP_MIN_SKIPPED, "finite": finite,
                             "colour_max": st["colour_max"], "colour_scale": packed.colour_scale}
        # the slice schedule of the frames to come (longer slices where few rays end: dsn_render_rays_ex), from the probe frame's histogram
        R_, S_ = getattr(self, "_probe_shape", (0, 0))
        if self.stop_schedule == "auto" and R_ > 0 and snap.numel() >= _lib.CNT_BYTES:
            hist, L = _lib.read_stop_hist(snap, R_, S_)
            lens, ev, un = _lib.choose_stop_schedule(hist, L, S_)
            if len(lens) < hist.shape[1]:
                packed.early_stop.update({"schedule": lens, "schedule_evaluates": ev, "uniform_evaluates": un})

    def _fit_records(self, positive_fraction, headroom=1.25):
        """the relu-record capacity of THIS renderer's workspaces (its own and its view slots') follows what its frames put on the
        sigma > 0 list; each workspace applies the request at the start of its next frame (RenderWorkspace.begin_frame) - never
        between the phases of a frame, and no other renderer's workspace is touched"""
        for ws in [self._ws] + [sl.ws for sl in self._slots if sl.ws is not self._ws]:
            ws.fit_records(positive_fraction, headroom)

    def _note_colour_max(self, packed, cmax, first=False):
        """the early-stop threshold's colour scale follows the largest colour seen: scale = 2 x that (never below 1, never lowered)"""
        if not (cmax == cmax) or cmax == float("inf"):
            # a NaN / inf colour reached a pixel: nothing sensible to scale with - termination off for these parameters
            if packed.early_stop is not None:
                packed.early_stop["usable"] = packed.early_stop["finite"] = False
            warnings.warn("dsnerf_amd: a frame weighed a non-finite colour: early stop stays off for these parameters")
            return
        want = _lib.EARLY_STOP_COLOUR_HEADROOM * cmax
        if first:
            if want > packed.colour_scale:
                packed.set_early_stop_colour_scale(want)
        elif cmax > packed.colour_scale:
            warnings.warn("dsnerf_amd: a sliced frame weighed colours up to %.3g, above the scale %.3g of the early-stop threshold (its "
                          "bound would be %.2g instead of 5e-5): the frame is rendered again in one pass, scale raised to %.3g"
                          % (cmax, packed.colour_scale, 5e-5 * cmax / packed.colour_scale, want))
            packed.set_early_stop_colour_scale(want)
            if packed.early_stop is not None:
                packed.early_stop["colour_scale"] = packed.colour_scale

    def _stop_guard(self, ws, scale, n_samples):
        """enqueue the copy of a sliced frame's counter words (largest colour weighed, samples on the sigma > 0 list) to page-locked
        memory behind the frame, on its stream: (host words, event, colour scale the frame's threshold used, samples, generation)"""
        pool = self._guard_pool
        host = pool.pop() if pool else torch.empty(256, dtype=torch.uint8).pin_memory()
        host.copy_(ws.buf[:256], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return (host, ev, float(scale), int(n_samples), self.net.packed(self.device).generation)

    def _stop_guards_ok(self, guards):
        """the hand-over check of sliced frames (waits for their counter copies - the frames themselves are done or about to be):
        True when every one of them stayed below the colour scale its threshold assumed.  Otherwise the scale is raised (warning) and
        the caller renders the frame again in one pass.  Also feeds the record capacity with what sliced frames really list."""
        ok = True
        packed = self.net.packed(self.device)
        for host, ev, scale, n_samples, gen in guards:
            ev.synchronize()
            c = host.view(torch.int32)
            cmax = float(c[_lib.CNT_COLOUR_MAX:_lib.CNT_COLOUR_MAX + 1].view(torch.float32)[0])
            n_pos = int(c[_lib.CNT_POS])
            self._guard_pool.append(host)
            if gen != packed.generation:
                continue
            if n_samples > 0:
                self._fit_records(n_pos / float(n_samples))
            if not (cmax <= scale):                       # (NaN / inf included)
                ok = False
                self._note_colour_max(packed, cmax)
        return ok

    def _hand_over(self, first, again, guards=None):
        """`first` is a frame that has been enqueued; before it goes to the caller the early-stop guards of its sliced render calls are
        looked at (their counter copies sit right behind the compositor on the frame's stream).  A frame that weighed a colour above
        the scale its threshold assumed is rendered AGAIN, in one pass (`again()`), and that is what the caller gets: the stated bound
        of early stop - 5e-5 absolute - then holds for every frame handed out, not only while the colours stay where the probe frame
        found them."""
        if guards is None:
            guards, self._guards = self._guards, []
        if not guards or self._stop_guards_ok(guards):
            return first
        self._one_pass_only = True
        try:
            res = again()
        finally:
            self._one_pass_only = False
            self._guards = []
        self.last_frame_info = dict(self.last_frame_info, rendered_again_in_one_pass=True)
        return res

    def last_screen_audit(self, ws=None):
        """what the audit of the last audited eval frame found - synchronises.  dict(audited, violations, max_sigma): `violations`
        audited samples (declared empty by the screen) have an accurate density > 0; they were rendered correctly (audited samples
        take the accurate pass), but their un-audited peers were not, so the screen is switched off for this renderer when it
        happens.  With screen_audit = "auto" this is the pending audited frame if there is one, else the last one judged."""
        if self.screen_audit == "auto":
            res = self._read_audit_probe(wait=True)
            return res if res is not None else getattr(self, "last_audit", None)
        ws = ws or self._ws
        if ws.buf is None:
            return None
        return self._judge_audit(ws.buf[:256].view(torch.int32).cpu())

    # Training steps whose activations / tangents / adjoints left the fp16 range of the split-fp16 kernels have no exact twin to fall
    # back to: the forward counts such samples (workspace word 48), the backward drops their second-order / adjoint terms and counts
    # them (dsn_train.hip, w.small[303]).  Both counters are copied to page-locked memory behind every backward and looked at -
    # without a wait - when the next step begins: a non-zero count is reported as a warning (nobody calls
    # range_overflow_count(), which synchronises).
    def _note_training_range(self, grad_word):
        st = getattr(self, "_range_watch", None)
        if st is None:
            st = self._range_watch = {"host": torch.zeros(2, dtype=torch.int32).pin_memory(), "ev": None, "warned": 0, "steps": 0}
        if st["ev"] is not None and not st["ev"].query():
            return                                    # the previous snapshot has not landed yet: skip this one
        self._poll_training_range()
        st["host"][0:1].copy_(self._ws.buf[4 * _lib.CNT_RANGE:4 * _lib.CNT_RANGE + 4].view(torch.int32), non_blocking=True)
        st["host"][1:2].copy_(grad_word, non_blocking=True)
        st["ev"] = torch.cuda.Event()
        st["ev"].record()

    def _poll_training_range(self):
        st = getattr(self, "_range_watch", None)
        if st is None or st["ev"] is None or not st["ev"].query():
            return
        st["ev"] = None
        fwd, bwd = int(st["host"][0]), int(st["host"][1])
        if fwd or bwd:
            st["steps"] += 1
            if st["warned"] < 5:
                st["warned"] += 1
                warnings.warn("dsnerf_amd: a training step had %d samples whose activations and %d whose tangents / adjoints left the "
                              "fp16 range of the split-fp16 kernels: their contributions to that step's gradients are not exact "
                              "(Renderer.range_overflow_count())" % (fwd, bwd))

    def range_overflow_count(self):
        """train mode: samples of the last render() whose activations / adjoints left the fp16 range of the split-fp16 kernels
        (there is no exact twin of the stored activations: a non-zero count means this step's gradients are not to be trusted;
        synchronises)."""
        if self._ws.buf is None:
            return 0
        return int(self._ws.buf[:256].view(torch.int32)[_lib.CNT_RANGE])

    # ---- whole-image path (reference :172-278) ----
    def batchify_rays_view(self, ray_o, ray_d, near, far, batch, chunk=None, scene=None, ws=None):
        scene = self.scene if scene is None else scene
        ws = self._ws if ws is None else ws
        # the frame's state first: its kernels (0.45 ms of nearest-face lists for the posed mesh) need the 82 KB of vertices only and
        # run while this thread stages the 8 MB of rays through page-locked memory (-0.1 ms per render_view, A/B in one call)
        self._set_frame(batch, scene=scene, lazy=True)
        screen = None
        pk = self.net.packed(self.device)
        if scene is not self.scene and pk.screen is not None:      # (not calibrated yet: _render_eval does it on this frame's points)
            screen = self.skip_transparent and not self.net.training and self.density_screen and pk.screen_pays(self._early_stop_in_use(pk))

        def render_chunk(o, d, n, f, S):
            jitter, noise = self._draws(o.shape[0], S)
            return self._render_eval(scene, ws, o, d, n, f, S, jitter, noise, screen=None if noise is not None else screen)
        return self._render_chunks(ray_o, ray_d, near, far, chunk, render_chunk), {}

    def _render_chunks(self, ray_o, ray_d, near, far, chunk, render_chunk, color_axis=0):
        """The view's rays on the device, rendered `chunk` rays at a time (None: all at once) by render_chunk(o, d, near, far, S)
        and joined along the ray axis (color_axis: that of "color", 1 for a sweep's [K, R, 3])."""
        o, d = self._dev(ray_o[0]), self._dev(ray_d[0])
        n, f = self._dev(near[0]).clone(), self._dev(far[0]).clone()
        S = self.cfg.MODEL.COARSE_RAY_SAMPLING
        R = o.shape[0]
        chunk = R if chunk is None else int(chunk)
        outs = []
        for i in range(0, R, chunk):
            j = min(R, i + chunk)
            outs.append(render_chunk(o[i:j].contiguous(), d[i:j].contiguous(), n[i:j].contiguous(), f[i:j].contiguous(), S))
        if len(outs) == 1:
            return outs[0]
        # ("shading" [K, R] of a maps sweep has its rays where a sweep's "color" has them)
        return {k: torch.cat([x[k] for x in outs], color_axis if k in ("color", "shading") else 0) for k in outs[0]}

    def _view_images(self, batch, chunk, scene, ws):
        coarse, _ = self.batchify_rays_view(batch["ray_o"], batch["ray_d"], batch["near"], batch["far"], batch, chunk, scene, ws)
        _, H, W, _ = batch["img"].shape
        # utils/render_utils.py:466-472 post_process, done on the device (dsn_image_scatter)
        return _lib.image_scatter(coarse, self._dev(batch["mask_at_box"][0], torch.uint8), H, W)

    def render_view(self, batch, chunk=None, device_output=False):
        """device_output=True (not in the reference) keeps the [H,W,*] images on the GPU - for multi-frame sequences
        (novel_pose_vis.py:41-66) and on-device metrics (`image_metrics`)."""
        with _HostPoolGuard(self.host_pool_limit):
            return self._render_view(batch, chunk, device_output)

    def _render_view(self, batch, chunk, device_output):
        img = self._view_images(batch, chunk, self.scene, self._ws)
        again = lambda: self._view_images(batch, chunk, self.scene, self._ws)
        if device_output:
            return self._hand_over(img, again)
        # four contiguous device images -> one persistent page-locked staging set (asynchronous copies, one synchronisation),
        # then fresh host tensors like the reference's `.cpu()` results.  A pageable `.cpu()` per image goes through the runtime's
        # own bounce buffers and varies between 1 and 20 ms per frame on the GPU boxes (scripts/d2h_probe.py);
        # `device_output=True` avoids the host side altogether.
        keys = ("coarse_color", "coarse_disp", "coarse_acc", "coarse_depth")
        stage = getattr(self, "_d2h_stage", None)
        if stage is None or any(stage[k].shape != img[k].shape for k in keys):
            stage = self._d2h_stage = {k: torch.empty(img[k].shape, dtype=torch.float32).pin_memory() for k in keys}
        for k in keys:
            stage[k].copy_(img[k], non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        checked = self._hand_over(img, again)      # (the guards' copies have landed with the images: no extra wait in the normal case)
        if checked is not img:
            for k in keys:
                stage[k].copy_(checked[k], non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
        # fresh pageable tensors (clone() of a page-locked tensor allocates page-locked memory again: 2-3 ms per image), copied
        # by one thread (see _dev)
        return {k: torch.from_numpy(stage[k].numpy().copy()) for k in keys}

    def render_view_lights(self, batch, lights, chunk=None, device_output=False):
        """render_view under several light settings from ONE geometry / field pass (not in the reference: its vis_lighting.py renders
        every view once per light).  `lights`: a list of dicts with the optional keys `light_center`, `rot`, `rot_center` - what
        net.set_light_center / set_rot / set_rot_center would set (rot and rot_center go together; {} = no light edit).  Returns one
        dict per light with render_view's keys; every image equals render_view's with that light set on the net.  The net's own
        light attributes are neither used nor changed; early stop, the density screen and its audit follow render_view's per-frame
        plan, and a sweep that weighed a colour above the early-stop scale under ANY light is rendered again in one pass
        (last_frame_info["rendered_again_in_one_pass"]).  Eval mode only.  Sampling, geometry, the field, the normals and the
        compositing weights run once; each light costs its lighting MLP and its rgb sums (dsn_render_rays_lights)."""
        lights = list(lights)
        if not lights:
            raise ValueError("render_view_lights: no lights given")
        if self.net.training:
            raise RuntimeError("render_view_lights: eval mode only (Renderer.eval()); a sweep has no training forward")
        if not self.skip_transparent:
            raise RuntimeError("render_view_lights: needs skip_transparent = True (the eval-mode path)")
        with _HostPoolGuard(self.host_pool_limit):
            imgs = self._view_images_lights(batch, lights, chunk)
            imgs = self._hand_over(imgs, lambda: self._view_images_lights(batch, lights, chunk))
            self.last_frame_info = dict(self.last_frame_info, lights=len(lights),
                                        rendered_again_in_one_pass=self.last_frame_info.get("rendered_again_in_one_pass", False))
            if device_output:
                return imgs
            torch.cuda.current_stream(self.device).synchronize()
            return [{k: v.cpu() for k, v in img.items()} for img in imgs]

    def _view_images_lights(self, batch, lights, chunk):
        scene, ws = self.scene, self._ws
        # the frame WITHOUT the net's light edit (fine_only=True, no light / rotation: each record of the sweep brings its own);
        # zero_code as DualSpaceNeRF.frame_args has it
        frame = int(torch.as_tensor(batch["frame"]).reshape(-1)[0])
        xyz = self._dev(batch["xyz"][0])
        poses = batch["poses"][0].to(device=self.device, dtype=torch.float32).contiguous()
        scene.set_frame(self.net.packed(self.device), xyz, poses, frame, self.net.nerf.w is not None, None, None, None, fine_only=True,
                        lazy=self.lazy_lists)
        self._frame_src = None      # (the scene's frame state now lacks the net's light edit: stage calls set their frame again)
        th = batch["Th"][0] if any(lt.get("light_center") is not None for lt in lights) else None
        recs = _lib.light_records(lights, th, self.device)
        coarse = self._render_chunks(batch["ray_o"], batch["ray_d"], batch["near"], batch["far"], chunk,
                                     lambda o, d, n, f, S: self._render_eval(scene, ws, o, d, n, f, S, None, None, lights=recs),
                                     color_axis=1)
        _, H, W, _ = batch["img"].shape
        mask = self._dev(batch["mask_at_box"][0], torch.uint8)
        return [_lib.image_scatter(dict(coarse, color=coarse["color"][k]), mask, H, W) for k in range(len(lights))]

    def render_view_maps(self, batch, lights=None, maps=("albedo", "shading", "normal"), chunk=None, device_output=False):
        """The decomposition behind a view (not in the reference, whose colour is (ELU(lighting MLP) + 1) x essence per sample,
        model/spacenet.py:174-188, and only ever composited as that product): the view's albedo, shading and normal images from the
        frame's own pass.  With w_i the frame's compositing weights, summed over the samples of its shading list:
            "albedo"  [H,W,3]  sum w_i essence_i        "shading" [H,W,1]  sum w_i (ELU + 1)_i
            "normal"  [H,W,3]  sum w_i n_i   (unit world normals; NOT renormalised: the acc-weighted mean normal x coarse_acc)
        zeros outside mask_at_box, beside render_view's four images.
        lights=None: the net's own light (light_center / rot / rot_center as set on the net) - ONE dict, its four render_view keys
        bit-identical to render_view(batch).  lights=[...] (render_view_lights' dicts): a list of dicts, one per light, colours
        bit-identical to render_view_lights; "albedo" / "normal" do not depend on the light and are the same tensors in every dict.
        maps: which of the three to produce.  Plan (early stop, density screen, audit, the second rendering in one pass when a colour
        above the early-stop scale was weighed) and restrictions as render_view_lights.  last_frame_info["maps"] names the maps; with
        early stop in use last_frame_info["maps_bound"] gives per map the absolute bound on its distance from the one-pass map,
        (S + 1) (eps + 2^-22) Q: Q = 1 for the normal (exact), the largest |essence| / light factor the frame weighed for albedo /
        shading - which bounds the samples early stop left out only as far as they are no larger than those it kept (the assumption
        the colour threshold itself makes)."""
        maps = (maps,) if isinstance(maps, str) else tuple(maps)
        if not maps:
            raise ValueError("render_view_maps: no maps asked for (albedo, shading, normal)")
        unknown = [m for m in maps if m not in _lib.MAPS]
        if unknown:
            raise ValueError(f"render_view_maps: unknown maps {unknown} (albedo, shading, normal)")
        single = lights is None
        if not single:
            lights = list(lights)
            if not lights:
                raise ValueError("render_view_maps: no lights given (None = the net's own light)")
        if self.net.training:
            raise RuntimeError("render_view_maps: eval mode only (Renderer.eval()); the maps have no training forward")
        if not self.skip_transparent:
            raise RuntimeError("render_view_maps: needs skip_transparent = True (the eval-mode path)")
        if single:
            net, own = self.net, {}
            if net.light_center is not None:
                own["light_center"] = net.light_center
            if net.rot is not None and net.rot_center is not None:      # (DualSpaceNeRF.frame_args: one without the other is ignored)
                own["rot"], own["rot_center"] = net.rot, net.rot_center
            lights = [own]
        with _HostPoolGuard(self.host_pool_limit):
            imgs, mx = self._view_images_maps(batch, lights, maps, chunk)
            res = self._hand_over((imgs, mx), lambda: self._view_images_maps(batch, lights, maps, chunk))
            imgs, mx = res
            info = dict(self.last_frame_info, lights=len(lights), maps=list(maps),
                        rendered_again_in_one_pass=self.last_frame_info.get("rendered_again_in_one_pass", False))
            if info.get("early_stop"):
                S = int(self.cfg.MODEL.COARSE_RAY_SAMPLING)
                e_max, l_max = (float(v) for v in mx.cpu())      # (synchronises; the hand-over check of a sliced frame has already)
                scale = {"albedo": e_max, "shading": l_max, "normal": 1.0}
                info["maps_max"] = {"essence": e_max, "light": l_max}
                info["maps_bound"] = {m: _lib.maps_bound(S, info["early_stop_eps"], scale[m]) for m in maps}
            self.last_frame_info = info
            if not device_output:
                torch.cuda.current_stream(self.device).synchronize()
                shared = {k: imgs[0][k].cpu() for k in ("albedo", "normal") if k in imgs[0]}
                imgs = [dict({k: v.cpu() for k, v in img.items() if k not in shared}, **shared) for img in imgs]
            return imgs[0] if single else imgs

    def _view_images_maps(self, batch, lights, maps, chunk):
        """_view_images_lights with the decomposition maps: (one dict per light, the [2] device tensor of the largest |essence| and
        light factor weighed)"""
        scene, ws = self.scene, self._ws
        frame = int(torch.as_tensor(batch["frame"]).reshape(-1)[0])
        xyz = self._dev(batch["xyz"][0])
        poses = batch["poses"][0].to(device=self.device, dtype=torch.float32).contiguous()
        scene.set_frame(self.net.packed(self.device), xyz, poses, frame, self.net.nerf.w is not None, None, None, None, fine_only=True,
                        lazy=self.lazy_lists)
        self._frame_src = None      # (as render_view_lights leaves it: the scene's frame state lacks the net's light edit)
        th = batch["Th"][0] if any(lt.get("light_center") is not None for lt in lights) else None
        recs = _lib.light_records(lights, th, self.device)
        coarse = self._render_chunks(batch["ray_o"], batch["ray_d"], batch["near"], batch["far"], chunk,
                                     lambda o, d, n, f, S: self._render_eval(scene, ws, o, d, n, f, S, None, None, lights=recs, maps=maps),
                                     color_axis=1)
        _, H, W, _ = batch["img"].shape
        mask = self._dev(batch["mask_at_box"][0], torch.uint8)
        K = len(lights)
        imgs = [_lib.image_scatter(dict(coarse, color=coarse["color"][k]), mask, H, W) for k in range(K)]
        rgbs = [coarse[m] for m in ("albedo", "normal") if m in maps]
        scal = [coarse["shading"][k] for k in range(K)] if "shading" in maps else []
        rgb_imgs, scal_imgs = _lib.image_scatter_maps(rgbs, scal, mask, H, W)
        for m, im in zip([m for m in ("albedo", "normal") if m in maps], rgb_imgs):
            for img in imgs:
                img[m] = im
        for img, im in zip(imgs, scal_imgs):
            img["shading"] = im
        return imgs, coarse["maps_max"].reshape(-1, 2).max(dim=0).values      # (one pair per chunk)

    def render_views(self, batches, frames_in_flight=3, device_output=True, chunk=None):
        """The per-frame loop of novel_pose_vis.py:41-66 / test.py:55-64 (`for batch in loader: render.render_view(batch)`) as
        ONE call over an iterable of batches, with `frames_in_flight` frames on their own HIP streams (own scene blob and
        workspace each): the per-frame setup, sampling and warp kernels of frame k+1 run beside the matrix-bound field kernels
        of frame k.  Returns the list of render_view results in order - bit-identical to calling render_view per batch.
        device_output=True keeps the images on the GPU (the D2H copies of host outputs are issued on each frame's stream and
        overlap the next frames too)."""
        with _HostPoolGuard(self.host_pool_limit):
            # (with frames overlapping, the persistent field kernels leave an eighth of the compute units to the neighbours' small
            #  kernels: DSN_SHARE_CUS, -1.4 % per frame; a frame alone keeps them all)
            self._frames_overlap = int(frames_in_flight) > 1
            try:
                return self._render_views(batches, frames_in_flight, device_output, chunk)
            finally:
                self._frames_overlap = False

    def _render_views(self, batches, frames_in_flight, device_output, chunk):
        n = max(1, int(frames_in_flight))
        while len(self._slots) < n:
            self._slots.append(_ViewSlot(self, own_scene=len(self._slots) > 0))
        slots = self._slots[:n]
        cur = torch.cuda.current_stream(self.device)
        self.net.packed(self.device)                         # shared, read-only state is materialised on the caller's stream
        self._t_vals(self.cfg.MODEL.COARSE_RAY_SAMPLING)
        # (the density screen is calibrated by the first frame itself, on its own points: _render_eval; slot 0 is the renderer's own
        #  scene and its frame is enqueued first)
        keys = ("coarse_color", "coarse_disp", "coarse_acc", "coarse_depth")
        results = []
        pending = []                       # (frame index, batch, its early-stop guards)
        self._guards = []
        for k, batch in enumerate(batches):
            slot = slots[k % n]
            slot.stream.wait_stream(cur)
            with torch.cuda.stream(slot.stream):
                img = self._view_images(batch, chunk, slot.scene, slot.ws)
                if self._guards:
                    pending.append((k, batch, self._guards))
                    self._guards = []
                if not device_output:
                    host = {kk: torch.empty(img[kk].shape, dtype=torch.float32).pin_memory() for kk in keys}
                    for kk in keys:
                        host[kk].copy_(img[kk], non_blocking=True)
                    results.append(host)
                else:
                    for t in img.values():
                        t.record_stream(cur)          # consumed on the caller's stream after the join below
                    results.append(img)
        for slot in slots:
            cur.wait_stream(slot.stream)
        if not device_output:
            torch.cuda.current_stream(self.device).synchronize()
        self._frame_src = None      # slot 0 shares the renderer's scene: it now holds the last frame slot 0 rendered
        # hand-over: every sliced frame's guard is looked at (this waits for the frames' compositors - the images of a device_output
        # call are then all but done); a frame that broke its bound is rendered again, alone, in one pass
        for k, batch, guards in pending:
            again = lambda b=batch: self._render_view(b, chunk, device_output)
            checked = self._hand_over(results[k], again, guards=guards)
            if checked is not results[k]:
                self._frame_src = None
                results[k] = checked
        return results

    def image_metrics(self, color_img, batch, clamp=True, ssim=False, lpips=None):
        """test.py:62-71 on the device: clamp to [0,1], psnr with and without mask_at_box against batch["img"].
        ssim=True adds "ssim": test.py:73-75's metrics.py ssim_metric of the same clamped image (dsn_image_ssim); it raises
        ValueError where skimage's compare_ssim would (a mask whose bounding rectangle is narrower or lower than 7 pixels).
        lpips={"alex": net, "vgg": net} (dsnerf_amd.lpips.LPIPS objects; either key alone will do) adds "lpips_alex" / "lpips_vgg":
        test.py:77-91's distances of the same clamped image (dsn_lpips); ValueError for a frame with a status (image below the
        net's smallest size, a non-finite pixel, the split-fp16 range left).
        Returns a dict of python floats (one device->host copy)."""
        img = color_img.to(self.device)
        if clamp:
            img = torch.clamp(img, min=0.0, max=1.0)
        gt = self._metrics_gt(batch)
        mask = self._dev(batch["mask_at_box"][0], torch.uint8)
        m = _lib.image_psnr(img, gt, mask)
        if ssim:
            s, rect, status = _lib.image_ssim(img, gt, mask.reshape(img.shape[:2]))
            m = torch.cat([m, s, status.double(), rect.reshape(-1).double()])
        names = self._lpips_names(lpips)
        for name in names:
            d, _, st = lpips[name].to(self.device).distance(img.to(torch.float32), gt)
            m = torch.cat([m, d, st.double()])
        return self._metrics_dicts(m[None].cpu(), lpips_names=names)[0]

    def image_metrics_views(self, images, batches, clamp=True, ssim=True, lpips=None):
        """image_metrics over a sequence: `images` are the [H,W,3] colour images of `batches` (e.g. the "coarse_color" tensors of
        render_views(batches, device_output=True)).  Frames of one size go through dsn_image_ssim (and, with lpips={"alex": net,
        "vgg": net}, dsn_lpips) together; psnr is dsn_image_psnr per frame; the whole sequence's numbers come back in ONE
        device->host copy.  Returns one dict per frame with image_metrics' keys; raises ValueError (naming the frame) where
        image_metrics would."""
        images, batches = list(images), list(batches)
        if len(images) != len(batches):
            raise ValueError(f"image_metrics_views: {len(images)} images for {len(batches)} batches")
        if not images:
            return []
        imgs, gts, masks = [], [], []
        for img, batch in zip(images, batches):
            img = img.to(self.device)
            imgs.append(torch.clamp(img, min=0.0, max=1.0) if clamp else img)
            gts.append(self._metrics_gt(batch))
            masks.append(self._dev(batch["mask_at_box"][0], torch.uint8).reshape(img.shape[:2]))
        rows = [None] * len(imgs)
        names = self._lpips_names(lpips)
        groups = {}
        for k, (img, gt) in enumerate(zip(imgs, gts)):
            groups.setdefault((tuple(img.shape), gt.dtype), []).append(k)
        for ks in groups.values():
            img = torch.stack([imgs[k] for k in ks]).contiguous()
            gt = torch.stack([gts[k] for k in ks]).contiguous()
            mask = torch.stack([masks[k] for k in ks]).contiguous()
            if ssim:
                s, rect, status = _lib.image_ssim(img, gt, mask)
            dist = [lpips[name].to(self.device).distance(img.to(torch.float32), gt) for name in names]
            for j, k in enumerate(ks):
                m = _lib.image_psnr(img[j], gt[j], mask[j])
                rows[k] = torch.cat([m, s[j:j + 1], status[j:j + 1].double(), rect[j].double()]) if ssim else m
                for d, _, st in dist:
                    rows[k] = torch.cat([rows[k], d[j:j + 1], st[j:j + 1].double()])
        return self._metrics_dicts(torch.stack(rows).cpu(), views=True, lpips_names=names)

    def save_views(self, results, paths, key="coarse_color", gt=None, clamp=False, **jpeg):
        """Write the device images of render_view(s)(device_output=True) as .jpg files (validate.py:76-83, novel_pose_vis.py:62-66,
        vis_lighting.py:62-65: `cv2.imwrite(path, img.numpy() * 255)`): `results` is one result dict or a list of them, `paths` one path
        per result.  The frames of one size are encoded in ONE dsnerf_amd.jpeg.encode call (two device->host copies per size group).
        key="coarse_color" writes three components from the B, G, R image; "coarse_depth" / "coarse_acc" / "coarse_disp" one
        component.  gt=batches puts batch["img"] to the right of the rendering (validate.py:78's np.concatenate(..., axis=1)),
        concatenated on the device.  clamp=True clamps to [0, 1] first (test.py:62); the encoder saturates either way.  **jpeg:
        quality, subsampling, channels, scale of jpeg.encode.  Returns the files' sizes in bytes."""
        from . import jpeg as _jpeg
        single = isinstance(results, dict)
        results = [results] if single else list(results)
        paths = [paths] if isinstance(paths, (str, os.PathLike)) else list(paths)
        if len(results) != len(paths):
            raise ValueError(f"save_views: {len(results)} results for {len(paths)} paths")
        for p in paths:
            if os.path.splitext(str(p))[1].lower() not in (".jpg", ".jpeg"):
                hint = " - save_views_png writes .png files" if os.path.splitext(str(p))[1].lower() == ".png" else ""
                raise ValueError(f"save_views: only .jpg / .jpeg files are written, got {p!r}{hint}")
        imgs = self._saved_images("save_views", results, key, gt, clamp)
        sizes = self._write_groups(imgs, paths, lambda stack: _jpeg.encode(stack, **jpeg))
        return sizes[0] if single else sizes

    def _saved_images(self, what, results, key, gt, clamp):
        """the device images save_views / save_views_png write: r[key] (one channel as [H, W]), clamped, with batch["img"] to its right"""
        if gt is not None:
            gt = [gt] if isinstance(gt, dict) else list(gt)
            if len(gt) != len(results):
                raise ValueError(f"{what}: {len(gt)} gt batches for {len(results)} results")
        imgs = []
        for k, r in enumerate(results):
            img = r[key].to(self.device)
            if img.dtype != torch.uint8:
                img = img.to(torch.float32)
            if img.dim() == 3 and img.shape[2] == 1:
                img = img[..., 0]
            if clamp:
                img = torch.clamp(img, min=0.0, max=1.0)
            if gt is not None:
                g = self._metrics_gt(gt[k]).to(torch.float32)
                if img.dim() == 2:
                    raise ValueError(f"{what}: gt goes beside a colour image, not beside " + key)
                img = torch.cat([img, g.reshape(img.shape[0], -1, 3)], dim=1)
            imgs.append(img)
        return imgs

    @staticmethod
    def _write_groups(imgs, paths, encode):
        """one encoder call per group of equal shape and dtype; the files' sizes in bytes"""
        groups = {}
        for k, img in enumerate(imgs):
            groups.setdefault((tuple(img.shape), img.dtype), []).append(k)
        sizes = [0] * len(imgs)
        for ks in groups.values():
            files = encode([imgs[k] for k in ks])
            for k, data in zip(ks, files):
                with open(paths[k], "wb") as f:
                    f.write(data)
                sizes[k] = len(data)
        return sizes

    def save_views_png(self, results, paths, key="coarse_color", gt=None, clamp=False, replicate=False, **png):
        """save_views for .png files (test.py:94-110), lossless: one dsnerf_amd.png.encode call per size group (two device->host copies
        each).  replicate=True writes a one-channel map ("coarse_depth", "coarse_acc") as three equal channels, test.py's
        np.repeat(..., 3, axis=2), without materialising them.  **png: channels, scale, filter, chunk of png.encode.  Returns the
        files' sizes in bytes."""
        from . import png as _png
        single = isinstance(results, dict)
        results = [results] if single else list(results)
        paths = [paths] if isinstance(paths, (str, os.PathLike)) else list(paths)
        if len(results) != len(paths):
            raise ValueError(f"save_views_png: {len(results)} results for {len(paths)} paths")
        for p in paths:
            if os.path.splitext(str(p))[1].lower() != ".png":
                raise ValueError(f"save_views_png: only .png files are written, got {p!r} (save_views writes .jpg files)")
        imgs = self._saved_images("save_views_png", results, key, gt, clamp)
        sizes = self._write_groups(imgs, paths, lambda stack: _png.encode(stack, replicate=replicate and stack[0].dim() == 2, **png))
        return sizes[0] if single else sizes

    TEST_VIEW_KINDS = ("img", "rendering", "gt", "depth", "acc")

    def save_test_views(self, results, batches, dirs, names, **png):
        """test.py:94-110's five .png files per evaluated frame: dirs maps "img" (rendering and ground truth side by side, H x 2 W),
        "rendering" (clamped to [0, 1] as test.py:62 does), "gt", "depth" and "acc" (the one-channel maps as three equal channels) to
        directories, names holds one file name per result (test.py's save_name); dirs[kind]/name.png is written.  Per frame size three
        encoder calls: the H x W colour images, the H x W maps, the H x 2 W pair joined on the device.  Returns {kind: [bytes per file]}."""
        from . import png as _png
        results = [results] if isinstance(results, dict) else list(results)
        batches = [batches] if isinstance(batches, dict) else list(batches)
        names = [names] if isinstance(names, str) else list(names)
        if not (len(results) == len(batches) == len(names)):
            raise ValueError(f"save_test_views: {len(results)} results, {len(batches)} batches, {len(names)} names")
        missing = [k for k in self.TEST_VIEW_KINDS if k not in dirs]
        if missing:
            raise ValueError(f"save_test_views: dirs needs the keys {self.TEST_VIEW_KINDS}, missing {missing}")
        path = {kind: [os.path.join(str(dirs[kind]), f"{n}.png") for n in names] for kind in self.TEST_VIEW_KINDS}
        colour = self._saved_images("save_test_views", results, "coarse_color", None, True)
        truth = [self._metrics_gt(b).to(torch.float32).reshape(c.shape) for b, c in zip(batches, colour)]
        pair = [torch.cat([c, g], dim=1) for c, g in zip(colour, truth)]
        depth = self._saved_images("save_test_views", results, "coarse_depth", None, False)
        acc = self._saved_images("save_test_views", results, "coarse_acc", None, False)
        n = len(results)
        flat = self._write_groups(colour + truth, path["rendering"] + path["gt"], lambda stack: _png.encode(stack, **png))
        maps = self._write_groups(depth + acc, path["depth"] + path["acc"], lambda stack: _png.encode(stack, replicate=True, **png))
        both = self._write_groups(pair, path["img"], lambda stack: _png.encode(stack, **png))
        return {"img": both, "rendering": flat[:n], "gt": flat[n:], "depth": maps[:n], "acc": maps[n:]}

    def _metrics_gt(self, batch):
        gt = batch["img"][0]
        return self._dev(gt, gt.dtype if gt.dtype in (torch.float32, torch.float64) else torch.float32)   # staged upload (6 MB of float64)

    @staticmethod
    def _lpips_names(lpips):
        if not lpips:
            return ()
        unknown = [k for k in lpips if k not in ("alex", "vgg")]
        if unknown:
            raise ValueError(f"lpips: the keys are 'alex' and 'vgg', got {unknown}")
        return tuple(k for k in ("alex", "vgg") if k in lpips)

    @staticmethod
    def _metrics_dicts(rows, views=False, lpips_names=()):
        """host rows {mse_all, mse_masked, psnr_all, psnr_masked[, ssim, status, x, y, w, h][, lpips, status per net]} ->
        image_metrics' dicts"""
        out = []
        for k, r in enumerate(rows.tolist()):
            d = {"mse": r[0], "mse_wMask": r[1], "psnr_woMask": r[2], "psnr_wMask": r[3]}
            tail = len(r) - 2 * len(lpips_names)
            if tail > 4:
                if int(r[5]) != _lib.SSIM_OK:
                    e = _lib.ssim_status_error(int(r[5]), r[6:10])
                    raise ValueError(f"frame {k}: {e}") if views else e
                d["ssim"] = r[4]
            for j, name in enumerate(lpips_names):
                value, status = r[tail + 2 * j], int(r[tail + 2 * j + 1])
                if status != _lib.LPIPS_OK:
                    e = ValueError(f"lpips_{name}: {_lib.lpips_status_text(status)}")
                    raise ValueError(f"frame {k}: {e}") if views else e
                d[f"lpips_{name}"] = value
            out.append(d)
        return out

    # ---- density grid + iso-surface on the device (utils/visualizer.py Visualizer3D, not in Renderer) ----
    @staticmethod
    def grid_axes(points, resolution):
        """Visualizer3D.get_grid's axes (utils/visualizer.py:170-227, eps = 0) as float64 numpy arrays (x, y, z): `resolution` points
        by linspace over the shortest extent of the points' bounding box, the other two by arange with that step"""
        p = points.detach().reshape(-1, 3).float().cpu().numpy() if torch.is_tensor(points) else np.asarray(points, np.float32).reshape(-1, 3)
        s = int(np.argmin(p.max(axis=0) - p.min(axis=0)))          # (float32 extents, as the reference's bounding_box)
        lo, hi = p.min(axis=0).astype(np.float64), p.max(axis=0).astype(np.float64)
        ax = [None] * 3
        ax[s] = np.linspace(lo[s], hi[s], int(resolution))
        step = (np.max(ax[s]) - np.min(ax[s])) / (ax[s].shape[0] - 1)
        for a in range(3):
            if a != s:
                ax[a] = np.arange(lo[a], hi[a] + step, step)
        return tuple(ax)

    @staticmethod
    def grid_axes_uniform(resolution):
        """Visualizer3D.get_grid_uniform's axes (utils/visualizer.py:238-251): linspace(-1.2, 1.2) on all three"""
        a = np.linspace(-1.2, 1.2, int(resolution))
        return a, a.copy(), a.copy()

    def density_grid(self, batch, resolution=None, axes=None, points=None, frame=None, fp32=False, slab_points=None):
        """Visualizer3D.get_grid_pred_batch's density volume on the device (dsn_density_grid): the grid of `axes` (default:
        grid_axes(points, resolution), points = batch["xyz"][0]) warped into the canonical space of batch's posed mesh, the density of
        every non-transparent point (0 elsewhere) with the frame code `frame` (default batch["frame"]; zeroed as
        DualSpaceNeRF.frame_args has it) and the pose of batch["poses"].  Returns (axes, volume [nx, ny, nz] device float32).
        fp32=True: the exact-fp32 kernel, i.e. the bits of query_volume(w2l_without_lbs(points)).  Render calls that follow set their
        own frame: their results do not change."""
        if axes is None:
            if resolution is None:
                raise ValueError("density_grid: give `resolution` or `axes`")
            axes = self.grid_axes(batch["xyz"][0] if points is None else points, resolution)
        self._ensure_mesh(batch)
        fi = int(torch.as_tensor(batch["frame"] if frame is None else frame).reshape(-1)[0])
        packed = self.net.packed(self.device)
        _lib.scene_set_pose(self.scene, packed, batch["poses"][0], fi, self.net.nerf.w is not None)
        self._frame_src = None          # (the scene's frame state now holds this pose code: stage calls set their frame again)
        vol = _lib.density_grid(self.scene, packed, axes, slab_points=slab_points, fp32=fp32)
        return axes, vol

    def density_grid_hier(self, batch, resolution=None, level=0.5, coarse=4, dilate=1, axes=None, points=None, frame=None, fp32=False,
                          slab_points=None):
        """density_grid's volume evaluated coarse to fine (dsn_grid_hier_* + dsn_density_points, the rule of include/dsnerf.h): the
        density on the sub-lattice of every `coarse`-th grid point (2, 4, 8 or 16), then only at the grid points in and around the
        coarse cells `level` crosses (`dilate` rings of cells around them); every other point holds a coarse value of its own side of
        the level.  Returns (axes, volume [nx, ny, nz] device float32, info): info = {factor, dilate, coarse_shape, core_cells,
        active_cells, evaluated_points, points, leaks}.  Evaluated points have density_grid's bits.
        info["leaks"] == 0 proves that every vertex and normal of marching cubes on this volume was computed from evaluated values
        only; where the volume also has the dense grid's inside mask, the mesh is the dense grid's, bit for bit.  It does not prove
        that nothing was missed: a piece of surface wholly among unevaluated points (a floater smaller than a coarse cell, more than
        `dilate` cells from any coarse sign change) is neither seen nor counted - largest_component would drop such pieces anyway."""
        if axes is None:
            if resolution is None:
                raise ValueError("density_grid_hier: give `resolution` or `axes`")
            axes = self.grid_axes(batch["xyz"][0] if points is None else points, resolution)
        self._ensure_mesh(batch)
        fi = int(torch.as_tensor(batch["frame"] if frame is None else frame).reshape(-1)[0])
        packed = self.net.packed(self.device)
        _lib.scene_set_pose(self.scene, packed, batch["poses"][0], fi, self.net.nerf.w is not None)
        self._frame_src = None          # (as density_grid: stage calls set their frame again)
        vol, info = _lib.density_grid_hier(self.scene, packed, axes, level, factor=coarse, dilate=dilate, slab_points=slab_points, fp32=fp32)
        return axes, vol, info

    def extract_mesh(self, batch, resolution=512, level=0.5, gradient_direction="ascent", axes=None, points=None, frame=None,
                     fp32=False, slab_points=None, normals=False, attributes=None, largest_component=False, simplify_cell=None,
                     target_vertices=None, smooth=None, coarse=None, dilate=1, max_dilate=3, report_distance=False):
        """Visualizer3D's mesh of the posed body on the device: density_grid + marching cubes (dsn_mc_count / dsn_mc_emit, the rule of
        include/dsnerf.h).  Defaults are the visualizer's __main__ values.  Returns {"verts" [V,3] float32, "faces" [T,3] int32} device
        tensors in world coordinates, or None where the level is not crossed (the reference returns None there).
        normals=True adds "normals" [V,3] float32, the unit vertex normals of dsn_mc_normals (along the density's gradient: out of the
        body with gradient_direction="descent", into it with "ascent", as the triangles of that mode are oriented); attributes: a tuple of mesh_attributes' names ("albedo", "normal", "colour", "sigma", "valid"), evaluated at the
        vertices with mesh_attributes' defaults and added under those names.  verts and faces do not depend on either.
        largest_component=True: only the connected component of the surface with the largest area (the reference visualizer's
        connected=True; dsn_mesh_cc_label / dsn_mesh_cc_emit, the rule of include/dsnerf.h) - floaters and inner shells go.  The
        filter runs right after marching cubes: the normals are gathered through "source_vertex" [V'] int32 (each kept vertex's index
        in the unfiltered mesh), the attributes are evaluated at the kept vertices only (per vertex and independent: the rows of
        the unfiltered call, bit for bit), and "n_components" says how many pieces the surface had.
        simplify_cell / target_vertices (one of them): the mesh thinned by vertex clustering (visualizer.simplify_mesh: dsn_mesh_simplify_count
        / dsn_mesh_simplify_emit, the rule of include/dsnerf.h) after the component filter and before the attributes, which are then
        evaluated at the few vertices that stay - input vertices, so again the rows of the unsimplified call.  The dict gains
        "cluster_source", "vertex_cluster" and "simplify_info"; normals and source_vertex are gathered.
        report_distance=True (with simplify_cell or target_vertices): the dict gains "distance", visualizer.mesh_distance(thinned mesh,
        the mesh before thinning) - how far the thinning moved the surface (dsn_mesh_dist_*, the rule of include/dsnerf.h).  Off by
        default; nothing else in the dict changes.
        smooth: an int (Taubin pairs) or a dict of visualizer.smooth_mesh's keywords - the stair steps of the thresholded grid smoothed
        out (dsn_mesh_smooth, the rule of include/dsnerf.h) after the component filter, before the thinning and before the attributes,
        which are then evaluated at the final vertices.  "normals" are then those of the smoothed faces (dsn_mesh_vertex_normals:
        oriented by the winding, which follows gradient_direction as marching cubes' do); the dict gains "smooth_info".
        coarse (2, 4, 8 or 16; None: the dense grid, as ever): the volume comes from density_grid_hier(coarse=coarse, dilate=dilate)
        - the density only near the iso-surface.  While the certificate fails (info["leaks"] > 0) and dilate < max_dilate the grid is
        built again with one more ring; if it still fails, the dense grid is used (hier_retry).  The dict gains "grid_info": the last
        attempt's info plus "attempts" and "fell_back".  With leaks == 0 every vertex and normal comes from evaluated densities; a
        floater smaller than a coarse cell and far from the surface can be missing (density_grid_hier's docstring).  Everything
        after marching cubes works on the result as before.  A field with structure below a coarse cell near the surface keeps the
        certificate from holding (the w4 body does, README): the call then costs the attempts plus the dense grid - look at grid_info."""
        if simplify_cell is not None and target_vertices is not None:
            raise ValueError("extract_mesh: give one of simplify_cell and target_vertices")
        if report_distance and simplify_cell is None and target_vertices is None:
            raise ValueError("extract_mesh: report_distance needs simplify_cell or target_vertices")
        names = tuple(attributes) if attributes else ()
        unknown = set(names) - set(self.MESH_ATTRIBUTES)
        if unknown:
            raise ValueError(f"extract_mesh: unknown attributes {sorted(unknown)} {self.MESH_ATTRIBUTES}")
        grid_info = None
        if coarse is None:
            axes, vol = self.density_grid(batch, resolution, axes, points, frame, fp32, slab_points)
        else:
            def attempt(r):
                a, v, info = self.density_grid_hier(batch, resolution, level, coarse, r, axes, points, frame, fp32, slab_points)
                return (a, v), info
            got, grid_info = hier_retry(attempt, dilate, max_dilate)
            axes, vol = got if got is not None else self.density_grid(batch, resolution, axes, points, frame, fp32, slab_points)
        out = _lib.marching_cubes(vol, axes, level, gradient_direction, want_normals=bool(normals))
        if out[1].shape[0] == 0:
            return None
        mesh = {"verts": out[0], "faces": out[1]}
        if normals:
            mesh["normals"] = out[2]
        if largest_component:
            info = {}
            v, f, src = _lib.largest_component(out[0], out[1], info=info)
            mesh.update(verts=v, faces=f, source_vertex=src, n_components=info["n_components"])
            if normals:
                mesh["normals"] = out[2][src.long()]
            out = (v, f)
        if smooth is not None:
            from .visualizer import smooth_keywords, smooth_mesh
            mesh = smooth_mesh(mesh, **smooth_keywords(smooth))
            out = (mesh["verts"], mesh["faces"])
        if simplify_cell is not None or target_vertices is not None:
            from .visualizer import mesh_distance, simplify_mesh
            mesh = simplify_mesh(mesh, cell=simplify_cell, target_vertices=target_vertices)
            if report_distance:
                mesh["distance"] = mesh_distance((mesh["verts"], mesh["faces"]), out)
            out = (mesh["verts"], mesh["faces"])
        if names:
            a = self.mesh_attributes(batch, out[0], frame=frame)
            mesh.update({k: a[k] for k in names})
        if grid_info is not None:
            mesh["grid_info"] = grid_info
        return mesh

    MESH_ATTRIBUTES = ("albedo", "normal", "colour", "sigma", "valid")
    MESH_VIEW_ORIGIN = (0.0, 0.0, 2.5)      # the translation of the mesh preview's default camera pose (_lib.raster_camera)

    @torch.no_grad()
    def mesh_attributes(self, batch, verts, view_origin=None, view_dirs=None, lights=None, frame=None, slab=1 << 22):
        """The field at the vertices of a mesh of batch's posed body (world coordinates, e.g. extract_mesh's): per slab of at most
        `slab` vertices dsn_warp (one sample per ray: per-vertex directions, an active list), dsn_field (essence and gradient of the
        listed vertices) and dsn_shade - the stage kernels as they are, so every value has the bits of those three calls, whatever
        the slab size.  The viewing direction of a vertex is verts - view_origin (default MESH_VIEW_ORIGIN), or view_dirs [V,3].
        Returns device tensors: "albedo" [V,3] (the essence), "normal" [V,3] (dsn_shade's unit world normal), "colour" [V,3]
        ((ELU + 1) x essence, the lit colour; with lights = [...] in render_view_lights' form [K,V,3]: dsn_shade once per light, the
        warp and the field once), "sigma" [V], "valid" [V] bool - False where the warp calls the vertex transparent; everything
        else is 0 there.  Frame, pose and code as density_grid takes them (no light edit of the net's applies without `lights`);
        the scene is left as density_grid leaves it, and render calls that follow set their own frame."""
        self._ensure_mesh(batch)
        fi = int(torch.as_tensor(batch["frame"] if frame is None else frame).reshape(-1)[0])
        packed = self.net.packed(self.device)
        poses, zero = batch["poses"][0], self.net.nerf.w is not None
        _lib.scene_set_pose(self.scene, packed, poses, fi, zero)
        self._frame_src = None          # (as density_grid: stage calls set their frame again)
        dev = self.device
        verts = torch.as_tensor(verts).to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
        V = verts.shape[0]
        if view_dirs is not None:
            dirs = torch.as_tensor(view_dirs).to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
            if dirs.shape[0] != V:
                raise ValueError(f"mesh_attributes: view_dirs has {dirs.shape[0]} rows for {V} vertices")
        else:
            o = torch.as_tensor(self.MESH_VIEW_ORIGIN if view_origin is None else view_origin)
            dirs = verts - o.to(device=dev, dtype=torch.float32).reshape(1, 3)
        recs = None
        if lights is not None:
            lights = list(lights)
            th = batch["Th"][0] if any(lt.get("light_center") is not None for lt in lights) else None
            recs = _lib.light_records(lights, th, "cpu")
        K = None if recs is None else recs.shape[0]
        out = {"albedo": torch.zeros(V, 3, device=dev), "normal": torch.zeros(V, 3, device=dev),
               "colour": torch.zeros((V, 3) if K is None else (K, V, 3), device=dev), "sigma": torch.zeros(V, device=dev),
               "valid": torch.zeros(V, dtype=torch.bool, device=dev)}
        slab = max(int(slab), 1)
        for s0 in range(0, V, slab):
            sl = slice(s0, min(s0 + slab, V))
            x_w, d = verts[sl].contiguous(), dirs[sl].contiguous()
            w = _lib.warp(self.scene, x_w, d, 1, want_dir=True, want_active=True)
            act = (w["active_list"], w["active_count"])
            sigma, ess, grad = _lib.field(self.scene, packed, w["x_c"], active=act)
            out["valid"][sl] = w["transparent"] == 0
            out["sigma"][sl], out["albedo"][sl] = sigma, ess
            if recs is None:
                _, out["normal"][sl], out["colour"][sl] = _lib.shade(self.scene, packed, w["x_c"], grad, x_w, d, ess, 1, active=act)
                continue
            for k in range(K):
                r = recs[k]
                _lib.scene_set_pose(self.scene, packed, poses, fi, zero, r[1:4] if r[0] else None, r[5:9] if r[4] else None,
                                    r[9:11] if r[4] else None)
                _, out["normal"][sl], out["colour"][k, sl] = _lib.shade(self.scene, packed, w["x_c"], grad, x_w, d, ess, 1, active=act)
        if recs is not None:
            _lib.scene_set_pose(self.scene, packed, poses, fi, zero)
        return out

    # ---- an extracted mesh under other poses (novel_pose_vis.py's animation, for the mesh: the rule of include/dsnerf.h) ----
    @torch.no_grad()
    def bind_mesh(self, batch, mesh, slab=1 << 22):
        """Bind a mesh of batch's posed body (world coordinates: extract_mesh's dict, or a (verts, faces[, normals]) tuple) to the
        body, once: per slab of at most `slab` vertices dsn_warp as it is (want_uvh), so every vertex keeps the record the warp gives
        a sample point there - "face_idx" [N] int32, "uv" [N,2], "h" [N], "valid" [N] bool (not transparent; reported only, the
        record is never clamped) and "x_c" [N,3], the warp's canonical position - whatever the slab size.  The mesh's "normals",
        where present, are bound with it: "cov" [N,3] (dsn_mesh_bind_normals; None without normals).  "verts" and "faces" are the
        bound mesh's own tensors, and every other entry of the mesh dict (albedo, colour, source_vertex, ...) is passed through
        untouched: vertex count and order never change under pose_mesh.  Frame state as mesh_attributes leaves it."""
        self._ensure_mesh(batch)
        fi = int(torch.as_tensor(batch["frame"]).reshape(-1)[0])
        _lib.scene_set_pose(self.scene, self.net.packed(self.device), batch["poses"][0], fi, self.net.nerf.w is not None)
        self._frame_src = None          # (as density_grid: stage calls set their frame again)
        dev = self.device
        if isinstance(mesh, dict):
            verts, faces, normals = mesh["verts"], mesh["faces"], mesh.get("normals")
        else:
            verts, faces, normals = (tuple(mesh) + (None,))[:3]
        verts = torch.as_tensor(verts).to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
        faces = torch.as_tensor(faces).to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()
        N = verts.shape[0]
        out = dict(mesh) if isinstance(mesh, dict) else {}
        out.update(face_idx=torch.empty(N, dtype=torch.int32, device=dev), uv=torch.empty(N, 2, device=dev), h=torch.empty(N, device=dev),
                   valid=torch.empty(N, dtype=torch.bool, device=dev), x_c=torch.empty(N, 3, device=dev), cov=None, verts=verts, faces=faces)
        slab = max(int(slab), 1)
        for s0 in range(0, N, slab):
            sl = slice(s0, min(s0 + slab, N))
            w = _lib.warp(self.scene, verts[sl].contiguous(), None, 1, want_dir=False, want_uvh=True)
            out["face_idx"][sl], out["uv"][sl], out["h"][sl], out["x_c"][sl] = w["face_idx"], w["uv"], w["h"], w["x_c"]
            out["valid"][sl] = w["transparent"] == 0
        if normals is not None:
            normals = torch.as_tensor(normals).to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
            if normals.shape[0] != N:
                raise ValueError(f"bind_mesh: {normals.shape[0]} normals for {N} vertices")
            out["cov"] = _lib.mesh_bind_normals(self._dev(batch["xyz"][0]).reshape(-1, 3), self.scene._keep[1], out["face_idx"], normals)
        return out

    @torch.no_grad()
    def pose_mesh(self, binding, targets, normals=True, stretch=False):
        """bind_mesh's binding under other bodies of the same topology (dsn_mesh_pose): `targets` is a tensor or array [P,Vb,3] or
        [Vb,3], a list of batches (each batch["xyz"][0]) or "canonical" (the renderer's canonical vertices: "verts" is then the
        binding's "x_c", bit for bit).  Returns device tensors {"verts" [P,N,3], "normals" [P,N,3] (None without bound normals or
        with normals=False), "stretch" [P,T] (dsn_mesh_stretch against the bound mesh; None unless stretch=True), "faces" [T,3]: the
        binding's own}; a [Vb,3] input or "canonical" gives unbatched shapes.  The triangle list is constant: where neighbouring
        vertices ride on different body parts a triangle tears, and visualizer.cull_stretched drops those by their stretch."""
        dev = self.device
        single = False
        if isinstance(targets, str):
            if targets != "canonical":
                raise ValueError(f"pose_mesh: unknown target {targets!r} (\"canonical\")")
            xyz, single = self.scene._keep[0][None], True
        elif isinstance(targets, (list, tuple)):
            if not targets:
                raise ValueError("pose_mesh: no target pose")
            xyz = torch.stack([self._dev(torch.as_tensor(t["xyz"][0] if isinstance(t, dict) else t)).reshape(-1, 3) for t in targets])
        else:
            xyz = torch.as_tensor(targets).to(device=dev, dtype=torch.float32)
            if xyz.dim() == 2:
                xyz, single = xyz[None], True
        if xyz.dim() != 3 or xyz.shape[2] != 3:
            raise ValueError(f"pose_mesh: targets must be [P,Vb,3] or [Vb,3], got {tuple(xyz.shape)}")
        if xyz.shape[1] != self.scene.V:
            raise ValueError(f"pose_mesh: a target body has {xyz.shape[1]} vertices, the renderer's body has {self.scene.V}")
        if xyz.shape[0] < 1:
            raise ValueError("pose_mesh: no target pose")
        o = _lib.mesh_pose(binding if normals else dict(binding, cov=None), self.scene._keep[1], xyz.contiguous())
        st = _lib.mesh_stretch(binding["verts"], o["verts"], binding["faces"]) if stretch else None
        pick = (lambda t: None if t is None else t[0]) if single else (lambda t: t)
        return {"verts": pick(o["verts"]), "normals": pick(o["normals"]), "stretch": pick(st), "faces": binding["faces"]}

    # ---- a motion clip without new_vertices/: the posed bodies and their view batches made on the device ----
    @torch.no_grad()
    def pose_body(self, model, poses, Rh=None, Th=None, pad="zju_eval"):
        """The posed bodies of a clip from its SMPL parameters (body.BodyModel.pose, dsn_body_pose): poses [P,24,3] or [P,72], Rh / Th
        [P,3] or None -> device tensors {"xyz" [P,V,3], "A" [P,24,4,4], "bounds" [P,2,3] (pad: "zju_eval" as the test split pads them,
        "zju_train", "h36m" or None), "Rh_mat" [P,3,3]} plus the inputs as given, on the device: "poses" [P,24,3], "Th" [P,3] (zeros
        without Th).  xyz[k][None] is a valid batch["xyz"], xyz a valid `targets` of pose_mesh / render_mesh_sequence, A[k] the
        joint_transforms of lbs_warp; view_batch() makes the whole batch of pose k."""
        if model.V != self.scene.V:
            raise ValueError(f"pose_body: the body model has {model.V} vertices, the renderer's body has {self.scene.V}")
        out = model.pose(poses, Rh=Rh, Th=Th, pad=pad, want=("xyz", "A", "bounds", "Rh_mat"))
        P = out["xyz"].shape[0]
        dev = out["xyz"].device
        out["poses"] = torch.as_tensor(poses).to(device=dev, dtype=torch.float32).reshape(P, 24, 3).contiguous()
        out["Th"] = (torch.zeros(P, 3, device=dev) if Th is None
                     else torch.as_tensor(Th).to(device=dev, dtype=torch.float32).reshape(P, 3).contiguous())
        return out

    @torch.no_grad()
    def view_batch(self, posed, k, K, R, T, H, W, poses=None, frame=0, convention="zju", **extra):
        """The batch render_view / render_views take for pose k of pose_body()'s result, seen by the camera K, R [3,3], T [3]: "xyz",
        "poses", "frame", "Th", "Rh", "bounds" of that pose, the rays of the H x W image against its bounds ("ray_o", "ray_d", "near",
        "far": the rays that meet the box, as the test split hands them over; "mask_at_box" [1,H*W]; _lib.camera_rays, convention "zju"
        or "h36m") and a zero "img" [1,H,W,3] for the image shape - everything on the device, nothing copied to the host.  The one
        wait is for the NUMBER of rays that meet the box, which sizes the compacted arrays (the frame's workspaces are sized from it
        on the host as well).  `poses`: the clip's [P,24,3] / [P,72] or pose k's own [24,3]; None: posed["poses"].  The use_x_pose edit
        of the pose the pose MLP sees (zju_mocap_dataset.py:76-78: poses[1,2] -= 0.6, poses[2,2] += 0.6) is the caller's, as it is
        with the datasets' batches: hand the edited poses over here.  `extra` entries are added as given."""
        k = int(k)
        P = posed["xyz"].shape[0]
        if not 0 <= k < P:
            raise IndexError(f"view_batch: pose {k} of {P}")
        dev = posed["xyz"].device
        bounds = posed["bounds"][k]
        ray_o, ray_d, near, far, mask = _lib.camera_rays(K, R, T, bounds, int(H), int(W), device=dev, convention=convention)
        poses = posed["poses"] if poses is None else torch.as_tensor(poses).to(device=dev, dtype=torch.float32)
        poses = poses.reshape(-1, 24, 3)
        pose = poses[0] if poses.shape[0] == 1 else poses[k]
        idx = mask.nonzero().reshape(-1)          # the one wait: its length comes to the host; the four gathers below need none
        ray_o, ray_d, near, far = (t.index_select(0, idx) for t in (ray_o, ray_d, near, far))
        batch = {"xyz": posed["xyz"][k][None], "poses": pose[None].contiguous(), "frame": torch.tensor([int(frame)]),
                 "Th": posed["Th"][k].reshape(1, 1, 3), "Rh": posed["Rh_mat"][k][None], "bounds": bounds[None],
                 "ray_o": ray_o[None], "ray_d": ray_d[None], "near": near[None], "far": far[None],
                 "mask_at_box": mask[None], "img": torch.zeros(1, int(H), int(W), 3, device=dev)}
        batch.update(extra)
        return batch

    # ---- density query for marching cubes (reference :280-296) ----
    def query_volume(self, pts, code_idx, transparent_mask=None, batch_info={}):
        """batch_info needs only 'poses' (the density-only branch of the reference, model/spacenet.py:223-241)."""
        B, N = pts.shape[:2]
        with torch.no_grad():
            density = self.net(pts, None, code_idx, batch_info, density_only=True)
        if transparent_mask is not None:
            density[transparent_mask.to(density.device).reshape([-1, 1])] = 0
        return density.reshape(B, N, 1)
