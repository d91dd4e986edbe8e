"""The catalogue behind tests/test_gpu_call_sequences.py: what a caller can ask of ONE Renderer between its construction and its end.

An OUTPUT operation takes (renderer, state) and returns a dict of named device tensors; a STATE operation changes the renderer or the
inputs of the calls that follow and returns nothing.  `state` is what the calls' inputs are built from: the body (Body: its vertices,
rays and training batch, fixed), which of its two poses is current, which of the two parameter sets (default, w4) the net holds, and
the pose tensor itself - the OBJECT batch["xyz"] is, because the renderer keys its posed mesh on that object.  Every operation sets
the mode (train / eval) and the draw source it needs and leaves them as it used them: nothing here tidies up after itself, so that
whatever a call leaves behind is what the next call meets.

The guarantee under test: an output operation's result is a function of (operation, pose, parameter set) alone - fresh_result() is
that function, evaluated on a Renderer that has done nothing else."""
import numpy as np
import torch

from cases import load, make_cfg, reference_loss, state as param_state

DEV = "cuda:0"
VIEW_KEYS = ("coarse_color", "coarse_disp", "coarse_acc", "coarse_depth")
PARAMS = ("default", "w4")
PSNR_KEYS = ("mse", "mse_wMask", "psnr_woMask", "psnr_wMask")
FUSED_MIN = 1 << 20            # = DSN_CELLMAJOR_MIN: from this many samples on the sampler classifies (tests/test_gpu_sampler_frame.py)
STAGE_MIN_BYTES = 1 << 16      # Renderer._dev: host tensors from this size on go through the page-locked staging ring


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


class Body:
    """one body with everything the operations feed to a renderer: two poses, per pose the rays of its views, the golden eval rays and
    the golden training batch (both made for pose 0 and used under either pose: any rays will do)"""

    def __init__(self, name):
        from dsnerf_amd import synth
        self.name = name
        small = name == "small"
        self.canon, self.faces = synth.make_small_body() if small else synth.make_body()
        ge, gt = load("small_eval" if small else "full_eval"), load("small_train_grads" if small else "full_train_grads")
        assert np.array_equal(ge["canonical_vertex"], self.canon) and np.array_equal(gt["canonical_vertex"], self.canon)
        self.S = int(ge["S"])
        assert self.S == int(gt["S"]) == (16 if small else 64)
        self.V = self.canon.shape[0]
        self.xyz = [synth.pose_body(self.canon, seed=3), synth.pose_body(self.canon, seed=23)]
        assert np.array_equal(self.xyz[0], ge["xyz"])
        self.poses = [synth.make_poses(seed=5), synth.make_poses(seed=41)]
        self.frame = [5, 9]
        self.th = np.array([0.2, -0.1, 1.0], np.float32)
        self.eval_rays = {k: ge[k].copy() for k in ("ray_o", "ray_d", "near", "far")}
        self.train = {k: gt[k].copy() for k in ("ray_o", "ray_d", "near", "far", "target_rgb", "occupancy")}
        self.train_seed, self.noise_std = int(gt["seed"]), float(gt["raw_noise_std"])
        # views: (H, W) of the main view, of render_views' second size and - full body - of the frame that reaches the fused classification
        self.view_hw = (37, 53) if small else (64, 64)
        self.second_hw = (24, 31) if small else (40, 48)
        self.fused_hw = None if small else (128, 128)
        self._views, self._skins = {}, {}
        rng = np.random.default_rng(7)
        self.points = [(x[rng.integers(0, self.V, 1500)] + rng.normal(0.0, 0.08, (1500, 3))).astype(np.float32) for x in self.xyz]
        self.mc_resolution = 40 if small else 56

    def skin(self, pose):
        """(verts, faces int32, unit vertex normals) of the posed body's triangles moved 1 cm out along the area-weighted normals"""
        if pose not in self._skins:
            x, f = self.xyz[pose].astype(np.float64), self.faces.astype(np.int64)
            fn = np.cross(x[f[:, 1]] - x[f[:, 0]], x[f[:, 2]] - x[f[:, 0]])
            n = np.zeros_like(x)
            for c in range(3):
                np.add.at(n, f[:, c], fn)
            n /= np.linalg.norm(n, axis=1, keepdims=True)
            self._skins[pose] = ((x + 0.01 * n).astype(np.float32), f.astype(np.int32), n.astype(np.float32))
        return self._skins[pose]

    def view(self, pose, hw):
        """rays, mask and ground truth of an H x W view of a pose: every tenth-or-so pixel is outside mask_at_box (a ragged ray count)"""
        from dsnerf_amd import synth
        key = (pose, hw)
        if key not in self._views:
            H, W = hw
            rays = synth.make_rays(H, W, self.xyz[pose], fit_box=True)
            assert rays["ray_o"].shape[0] == H * W
            mask = synth.hash_uniform(H * W, 700 + pose) >= 0.09
            if hw == self.fused_hw:
                mask[:] = True
            y, x = np.mgrid[0:H, 0:W]
            img = np.stack([(x + k * y + 3 * pose) % 17 / 16.0 for k in range(3)], -1)          # float64 [H, W, 3]
            self._views[key] = ({k: rays[k][mask] for k in ("ray_o", "ray_d", "near", "far")}, mask, img)
        return self._views[key]


_BODIES = {}


def body(name):
    if name not in _BODIES:
        _BODIES[name] = Body(name)
    return _BODIES[name]


# ---- state and renderers --------------------------------------------------------------------------------------------------------
def new_state(b, pose=0, params="default"):
    return {"body": b, "pose": pose, "params": params, "xyz": _t(b.xyz[pose].copy())[None]}


def describe(state):
    return "pose %d, %s parameters" % (state["pose"], state["params"])


def _state_dict(params):
    return {k: _t(v) for k, v in param_state("x_w4" if params == "w4" else None).items()}


def new_renderer(b, params="default", early_stop=False):
    import dsnerf_amd
    cfg = make_cfg(b.S)
    cfg.MODEL.raw_noise_std = b.noise_std
    net = dsnerf_amd.DualSpaceNeRF(cfg)
    net.load_state_dict(_state_dict(params))
    net.cuda()
    r = dsnerf_amd.Renderer(net, None, cfg, _t(b.canon), body_data={"f": b.faces})
    r.early_stop = early_stop
    r.eval()
    return r


def frame_batch(state, pose=None, xyz=None):
    """the frame part of a batch: the CURRENT pose with the state's own pose tensor, or another pose with a tensor of its own"""
    b = state["body"]
    p = state["pose"] if pose is None else pose
    if xyz is None:
        xyz = state["xyz"] if p == state["pose"] else _t(b.xyz[p].copy())[None]
    return {"xyz": xyz, "poses": _t(b.poses[p])[None], "Th": _t(b.th).reshape(1, 1, 3), "frame": torch.tensor([b.frame[p]])}


def ray_batch(state, rays):
    out = frame_batch(state)
    out.update({k: _t(rays[k].copy())[None] for k in ("ray_o", "ray_d", "near", "far")})
    return out


def view_batch(state, hw=None, pose=None):
    b = state["body"]
    p = state["pose"] if pose is None else pose
    rays, mask, img = b.view(p, b.view_hw if hw is None else hw)
    out = frame_batch(state, pose=p)
    out.update({k: _t(rays[k].copy())[None] for k in ("ray_o", "ray_d", "near", "far")})
    out["mask_at_box"] = _t(mask)[None]
    out["img"] = _t(img)[None]
    return out


def _keep(d, keys=None, prefix=""):
    return {prefix + k: d[k].detach().clone() for k in (d if keys is None else keys) if torch.is_tensor(d[k])}


def _scalars(d, keys):
    return {k: torch.tensor([float(d[k])], dtype=torch.float64) for k in keys}


# ---- output operations ------------------------------------------------------------------------------------------------------
def op_render(r, state):
    """Renderer.render of the golden rays, eval mode"""
    r.eval()
    return _keep(r.render(ray_batch(state, state["body"].eval_rays))["coarse"])


def op_view(r, state):
    """render_view, whole, host outputs (the page-locked image staging set)"""
    r.eval()
    out = r.render_view(view_batch(state))
    assert not out["coarse_color"].is_cuda
    return {k: out[k].to(DEV) for k in VIEW_KEYS}


def op_view_chunked(r, state):
    """render_view with a chunk that does not divide R"""
    r.eval()
    b = view_batch(state)
    R = b["ray_o"].shape[1]
    chunk = R // 3 + 5
    assert R % chunk != 0 and chunk < R
    return _keep(r.render_view(b, chunk=chunk, device_output=True), VIEW_KEYS)


def op_view_fused(r, state):
    """full body only: the 128 x 128 view, R S = 2^20 samples - the sampler classifies (the fused geometry phase)"""
    b = state["body"]
    r.eval()
    vb = view_batch(state, hw=b.fused_hw)
    n = vb["ray_o"].shape[1] * b.S
    assert n >= FUSED_MIN, n
    assert vb["ray_o"].numel() * 4 >= STAGE_MIN_BYTES and state["xyz"].numel() * 4 >= STAGE_MIN_BYTES      # (both through the staging ring)
    return _keep(r.render_view(vb, device_output=True), VIEW_KEYS)


def op_views(r, state):
    """render_views(frames_in_flight=3) over four batches of two sizes, the larger first; the third one shows the other pose"""
    b = state["body"]
    r.eval()
    other = 1 - state["pose"]
    batches = [view_batch(state), view_batch(state, hw=b.second_hw), view_batch(state, pose=other), view_batch(state, hw=b.second_hw)]
    assert batches[0]["ray_o"].shape[1] > batches[1]["ray_o"].shape[1]
    res = r.render_views(batches, frames_in_flight=3, device_output=True)
    out = {}
    for i, v in enumerate(res):
        out.update(_keep(v, VIEW_KEYS, prefix="%d:" % i))
    return out


def _angle2rot(angle):                                              # vis_lighting.py:86-91
    rad = np.pi * angle / 180
    return torch.Tensor(np.array([[np.cos(rad), -np.sin(rad)], [np.sin(rad), np.cos(rad)]]))


def five_lights():
    """no edit, a shifted light, a rotation about the head, both, a light far away (the five of tests/test_gpu_relight.py)"""
    head = torch.tensor([[0.18649693, -0.14180326, 1.7103844]])
    return [{}, {"light_center": torch.tensor([0.35, 0.05, 1.4])}, {"rot": _angle2rot(72), "rot_center": head},
            {"light_center": torch.tensor([-0.3, 0.4, 0.9]), "rot": _angle2rot(252), "rot_center": head},
            {"light_center": torch.tensor([6.0, -4.0, 9.0])}]


def op_view_lights(r, state):
    """render_view_lights with 5 lights"""
    r.eval()
    res = r.render_view_lights(view_batch(state), five_lights(), device_output=True)
    assert len(res) == 5
    out = {}
    for i, v in enumerate(res):
        out.update(_keep(v, VIEW_KEYS, prefix="light%d:" % i))
    return out


def op_view_maps(r, state):
    """render_view_maps (the net's own light)"""
    r.eval()
    return _keep(r.render_view_maps(view_batch(state), device_output=True), VIEW_KEYS + ("albedo", "shading", "normal"))


def _train_forward(r, state):
    b = state["body"]
    r.train()
    r.net.zero_grad(set_to_none=True)
    return r.render(ray_batch(state, b.train))["coarse"]


def _train_backward(r, state, out):
    b = state["body"]
    fwd = _keep(out, ("color", "disp_map", "acc_map", "depth_map", "weights", "z_vals"), prefix="out:")
    loss = reference_loss(out, _t(b.train["target_rgb"]).to(DEV), _t(b.train["occupancy"]).to(DEV))
    loss.backward()
    fwd["loss"] = loss.detach().reshape(1).clone()
    for k, p in r.net.named_parameters():
        assert p.grad is not None, k
        fwd["grad:" + k] = p.grad.detach().clone()
    r.net.zero_grad(set_to_none=True)
    return fwd


def op_train_host(r, state):
    """train-mode render + reference_loss + backward, the draws from the host generator seeded here"""
    r.draws = "host"
    torch.manual_seed(state["body"].train_seed)
    return _train_backward(r, state, _train_forward(r, state))


def op_train_device(r, state):
    """the same with draws = "device" after seed_draws"""
    r.draws = "device"
    r.seed_draws(0x5EED1234, step=7)
    return _train_backward(r, state, _train_forward(r, state))


def op_train_deferred(r, state):
    """a train forward whose backward runs only after an eval frame of the OTHER pose went through the same scene (the backward sets
    its frame again: Scene.set_frame(reuse=True) must not take the eval frame for its own)"""
    r.draws = "host"
    torch.manual_seed(state["body"].train_seed + 1)
    out = _train_forward(r, state)
    r.eval()
    between = r.render_view(view_batch(state, hw=state["body"].second_hw, pose=1 - state["pose"]), device_output=True)
    res = _train_backward(r, state, out)
    res.update(_keep(between, VIEW_KEYS, prefix="between:"))
    return res


def op_w2l(r, state):
    """w2l_without_lbs on arbitrary points with a batch that holds the pose tensor only (utils/visualizer.py's call)"""
    b = state["body"]
    r.eval()
    pts = _t(b.points[state["pose"]]).reshape(1, 50, 30, 3)
    x_c, mask = r.w2l_without_lbs(pts, {"xyz": state["xyz"]}, r.canonical_model)
    return {"x_c": x_c.clone(), "transparent": mask.to(torch.uint8).clone()}


def op_query_volume(r, state):
    """query_volume on canonical points (the density-only forward)"""
    b = state["body"]
    r.eval()
    p = state["pose"]
    pts = _t((b.canon[::max(1, b.V // 700)] * 0.97).astype(np.float32))[None]
    mask = _t(np.arange(pts.shape[1]) % 11 == 0)[None]
    q = r.query_volume(pts, torch.tensor([b.frame[p]]), mask, {"poses": _t(b.poses[p])[None]})
    return {"density": q.clone()}


def op_density_grid(r, state):
    """density_grid(resolution=24)"""
    r.eval()
    axes, vol = r.density_grid(frame_batch(state), resolution=24)
    return {"volume": vol.clone(), "shape": torch.tensor(vol.shape, dtype=torch.int32)}


def _mesh_tensors(mesh):
    if mesh is None:
        return {"no_surface": torch.ones(1, dtype=torch.int32)}
    out = _keep(mesh)
    out["n_components"] = torch.tensor([int(mesh["n_components"])], dtype=torch.int32)
    gi = mesh["grid_info"]
    out["grid_info"] = torch.tensor([int(gi["attempts"]), int(gi["fell_back"]), int(gi["leaks"]), int(gi["evaluated_points"])], dtype=torch.int64)
    return out


def op_extract_mesh(r, state):
    """extract_mesh coarse to fine, largest component, smoothed, thinned, with an attribute"""
    r.eval()
    mesh = r.extract_mesh(frame_batch(state), resolution=state["body"].mc_resolution, coarse=4, largest_component=True, smooth=2,
                          target_vertices=300, attributes=("albedo",))
    return _mesh_tensors(mesh)


def _skin(state):
    """a closed mesh around the current pose: the posed body's own triangles, 1 cm out along the vertex normals (made on the host)"""
    v, f, n = state["body"].skin(state["pose"])
    return _t(v).to(DEV), _t(f).to(DEV), _t(n).to(DEV)


def op_bind_pose_mesh(r, state):
    """bind_mesh + pose_mesh: a mesh around the current pose bound once, then carried to the other pose and to the canonical body"""
    b = state["body"]
    r.eval()
    v, f, n = _skin(state)
    binding = r.bind_mesh(frame_batch(state), {"verts": v, "faces": f, "normals": n})
    posed = r.pose_mesh(binding, _t(b.xyz[1 - state["pose"]]), stretch=True)
    canon = r.pose_mesh(binding, "canonical")
    out = _keep(binding, ("face_idx", "uv", "h", "valid", "x_c", "cov"), prefix="bind:")
    out.update(_keep(posed, ("verts", "normals", "stretch"), prefix="posed:"))
    out.update(_keep(canon, ("verts", "normals"), prefix="canon:"))
    return out


def op_mesh_preview(r, state):
    """the mesh preview raster (smooth shading, vertex colours) of the mesh around the current pose"""
    from dsnerf_amd import _lib
    r.eval()
    v, f, n = _skin(state)
    c = v.mean(0).cpu().numpy().astype(np.float64)
    pose = np.eye(4)
    pose[:3, 3] = c + np.array([0.0, 0.0, 2.5])
    colours = (v - v.min(0).values) / (v.max(0).values - v.min(0).values)
    out = _lib.raster_mesh(v, f, camera_pose=pose, height=96, width=80, vertex_normals=n, vertex_colors=colours.contiguous(), smooth=True)
    return _keep(out, ("color", "depth", "face", "normal", "attr"))


def op_image_metrics(r, state):
    """image_metrics(ssim=True) of a rendered view"""
    r.eval()
    b = view_batch(state)
    img = r.render_view(b, device_output=True)["coarse_color"]
    m = r.image_metrics(img, b, ssim=True)
    return _scalars(m, sorted(k for k in m if isinstance(m[k], (int, float))))


def _rendered_colour(r, state):
    r.eval()
    return r.render_view(view_batch(state), device_output=True)["coarse_color"]


def op_jpeg(r, state):
    """jpeg.encode -> jpeg.decode of a rendered frame, on the renderer's stream"""
    from dsnerf_amd import jpeg
    img = _rendered_colour(r, state)
    data = jpeg.encode(img, quality=90)
    px = jpeg.decode(data[0])
    return {"file": torch.frombuffer(bytearray(data[0]), dtype=torch.uint8).clone(), "pixels": px.clone()}


def op_png(r, state):
    """png.encode -> png.decode of a rendered frame, on the renderer's stream"""
    from dsnerf_amd import png
    img = _rendered_colour(r, state)
    data = png.encode(img)
    px = png.decode(data[0])
    return {"file": torch.frombuffer(bytearray(data[0]), dtype=torch.uint8).clone(), "pixels": px.clone()}


OUTPUT_OPS = {
    "render": op_render, "view": op_view, "view_chunked": op_view_chunked, "views": op_views, "train_host": op_train_host, "train_device": op_train_device, "train_deferred": op_train_deferred,
    "w2l": op_w2l, "query_volume": op_query_volume, "density_grid": op_density_grid, "extract_mesh": op_extract_mesh,
    "bind_pose_mesh": op_bind_pose_mesh, "mesh_preview": op_mesh_preview, "image_metrics": op_image_metrics, "jpeg": op_jpeg,
    "png": op_png,
}
# the sweeps run on the 16-lane compositor, which takes S = 64 or 128: the small body's S = 16 renderer refuses them with an error
FULL_ONLY_OPS = {"view_lights": op_view_lights, "view_maps": op_view_maps, "view_fused": op_view_fused}


def op_view_device(r, state):
    """render_view, whole, device outputs: the frame the early-stop walk slices (not part of the pair walks: `view` and `view_chunked`
    already are)"""
    r.eval()
    return _keep(r.render_view(view_batch(state), device_output=True), VIEW_KEYS)


EXTRA_OPS = {"view_device": op_view_device}


# the operations by family (the fresh table is filled a family at a time)
FAMILIES = {
    "views": ("render", "view", "view_chunked", "views", "view_lights", "view_maps", "view_fused", "view_device"),
    "training": ("train_host", "train_device", "train_deferred"),
    "stages": ("w2l", "query_volume", "density_grid"),
    "meshes": ("extract_mesh", "bind_pose_mesh", "mesh_preview"),
    "metrics_and_codecs": ("image_metrics", "jpeg", "png"),
}
assert sorted(n for f in FAMILIES.values() for n in f) == sorted(list(OUTPUT_OPS) + list(FULL_ONLY_OPS) + list(EXTRA_OPS))


def output_ops(b):
    """the output operations of a body (b: a Body or its name), in catalogue order"""
    ops = dict(OUTPUT_OPS)
    if (b if isinstance(b, str) else b.name) == "full":
        ops.update(FULL_ONLY_OPS)
    return ops


def any_op(b, name):
    return output_ops(b).get(name) or EXTRA_OPS.get(name) or STATE_OPS[name]


# ---- state operations -------------------------------------------------------------------------------------------------------
def st_pose_new(r, state):
    """the other pose, as a new tensor"""
    b = state["body"]
    state["pose"] = 1 - state["pose"]
    state["xyz"] = _t(b.xyz[state["pose"]].copy())[None]


def st_pose_in_place(r, state):
    """the other pose written into the same tensor (same object, same address, new version)"""
    b = state["body"]
    state["pose"] = 1 - state["pose"]
    state["xyz"].copy_(_t(b.xyz[state["pose"]])[None])


def st_pose_freed_address(r, state):
    """the other pose in a NEW tensor at the freed address of the old one, if the allocator hands it out again within 64 tries"""
    b = state["body"]
    shape = tuple(state["xyz"].shape)
    ptr = state["xyz"].data_ptr()
    del state["xyz"]
    tried, new = [], None
    for _ in range(64):
        cand = torch.empty(shape)
        if cand.data_ptr() == ptr:
            new = cand
            break
        tried.append(cand)                 # (kept until the loop ends: a freed candidate would only come back itself)
    if new is None:
        new = torch.empty(shape)           # could not provoke the reuse: a new tensor all the same
    del tried
    state["pose"] = 1 - state["pose"]
    new.copy_(_t(b.xyz[state["pose"]])[None])
    state["xyz"] = new
    state["address_reused"] = state.get("address_reused", 0) + int(new.data_ptr() == ptr)


def _load_params(r, state, params):
    """a parameter set loaded into the same net, in place: the parameters' versions move, and with them packed.generation at the next
    call that asks for the packed image (nothing is re-packed here: the next operation meets the stale image)"""
    before = [p._version for p in r.net.parameters()]
    state["params"] = params
    r.net.load_state_dict(_state_dict(params))
    assert all(p._version > v for p, v in zip(r.net.parameters(), before))


def st_params_w4(r, state):
    """the w4 parameters loaded into the net (again, if it holds them: the generation moves either way)"""
    _load_params(r, state, "w4")


def st_params_default(r, state):
    """the default parameters loaded into the net"""
    _load_params(r, state, "default")


def st_train_mode(r, state):
    """train().  Every output operation sets the mode it needs as its first action, so what this couple shows is only that train()
    itself leaves nothing behind; the modes that matter are crossed by the pair walk (a training step in front of every call)"""
    r.train()


def st_eval_mode(r, state):
    """eval() (see st_train_mode)"""
    r.eval()


def st_lazy_off(r, state):
    """lazy_lists and train_lazy_lists off: every cell's lists are built when the frame is set"""
    r.lazy_lists = r.train_lazy_lists = False


def st_lazy_on(r, state):
    """lazy_lists and train_lazy_lists on (the default)"""
    r.lazy_lists = r.train_lazy_lists = True


def st_screen_on(r, state):
    """density_screen = True with screen_audit = True"""
    r.density_screen, r.screen_audit = True, True


def st_screen_off(r, state):
    """the density screen and its audit back to the defaults"""
    r.density_screen, r.screen_audit = False, "auto"


# (order matters to the pair walk's state section: the default parameters are loaded last, so the screen - which the w4 parameters
#  calibrate as unsafe - is switched on in front of every operation while the net holds parameters it engages for)
STATE_OPS = {"pose_new": st_pose_new, "pose_in_place": st_pose_in_place, "pose_freed_address": st_pose_freed_address,
             "params_w4": st_params_w4, "params_default": st_params_default, "train_mode": st_train_mode, "eval_mode": st_eval_mode,
             "lazy_off": st_lazy_off, "lazy_on": st_lazy_on, "screen_on": st_screen_on, "screen_off": st_screen_off}
# the operations that render an eval frame through Renderer._render_eval and so leave last_frame_info["density_screen"]
EVAL_FRAME_OPS = ("render", "view", "view_chunked", "views", "view_lights", "view_maps", "view_fused", "view_device", "image_metrics",
                  "jpeg", "png")


# ---- the fresh side ---------------------------------------------------------------------------------------------------------
def fresh_result(b, name, pose, params, before=()):
    """operation `name` on a newly constructed Renderer with its own Scene, PackedParams and workspace that starts at (pose, params)
    and first runs the operations `before` - none for the fresh table; the failure message's [previous, operation] check passes one"""
    r = new_renderer(b, params)
    state = new_state(b, pose, params)
    for prev in before:
        any_op(b, prev)(r, state)
    out = any_op(b, name)(r, state)
    torch.cuda.synchronize()
    return out


# ---- the comparison rule ----------------------------------------------------------------------------------------------------
def words(t):
    """a tensor's raw content as integers: int32 words where the element size allows (NaN in disp is legitimate: compare bits)"""
    t = t.detach().contiguous().reshape(-1)
    if t.element_size() % 4 == 0:
        return t.view(torch.int32)
    return t.view(torch.uint8)


FLOOR = 2e-6          # = tests/test_gpu_train.py's FLOOR (the test module asserts that it is)
# The gradient tensors two FRESH renderers were seen to disagree on (float atomics in the head products), per body - every run of
# test_two_fresh_renderers_agree on the MI355X, 1 to 830 differing words, at most 2.2e-7 relative L2 (docs/LAB_NOTEBOOK.md R15).
# On the small body (64 rays x 16 samples) only three of them ever differed.  Every other gradient - the trunk, the embedding, the
# pose MLP, rgb_net.1, lights_encoding.2 - was the same bits in every pair of fresh renderers and is compared bit for bit.
LOOSE_GRADS = {
    "small": ("lighting_mlp.lights_encoding.0.weight", "lighting_mlp.lights_encoding.0.bias", "nerf.density_net.0.weight"),
    "full": ("lighting_mlp.lights_encoding.0.weight", "lighting_mlp.lights_encoding.0.bias", "lighting_mlp.lights_encoding.4.weight",
             "lighting_mlp.lights_encoding.4.bias", "nerf.density_net.0.weight", "nerf.density_net.0.bias", "nerf.rgb_net.3.weight",
             "nerf.rgb_net.3.bias"),
}


def tolerance_of(key, body):
    """None: bit for bit.  The two quantities two FRESH renderers already disagree on (float atomics), each with the bar the suite
    already uses for it: ("rel", 1e-12) dsn_image_psnr's four keys (tests/test_gpu_lpips.py), ("l2", FLOOR) the gradients listed in
    LOOSE_GRADS for the body (tests/test_gpu_train.py's bar for the head products)"""
    if key in PSNR_KEYS:
        return ("rel", 1e-12)
    if key.startswith("grad:") and key[5:] in LOOSE_GRADS[body]:
        return ("l2", FLOOR)
    return None


def difference(key, got, want, body):
    """None where `got` passes for `want` under the rule, else (differing words or elements, a short description)"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return (max(got.numel(), want.numel()), "shape / dtype %s %s against %s %s" % (tuple(got.shape), got.dtype, tuple(want.shape), want.dtype))
    want = want.to(got.device)
    tol = tolerance_of(key, body)
    if tol is None:
        n = int((words(got) != words(want)).sum())
        return None if n == 0 else (n, "%d of %d words differ" % (n, words(got).numel()))
    a, w = got.double(), want.double()
    if tol[0] == "rel":
        bad = ~((a - w).abs() <= tol[1] * w.abs())          # (NaN on either side is a difference)
        n = int(bad.sum())
        return None if n == 0 else (n, "relative difference %.3g (bar %.1g)" % (float(((a - w).abs() / w.abs()).max()), tol[1]))
    d = float((a - w).norm() / w.norm().clamp_min(1e-300))
    return None if d <= tol[1] else (int((a != w).sum()), "relative L2 difference %.3g (bar %.1g)" % (d, tol[1]))


def first_difference(got, want, body):
    """None, or (key, count, description) of the first key (sorted) of two result dicts that differs under the body's rule"""
    if sorted(got) != sorted(want):
        return ("<keys>", len(set(got) ^ set(want)), "keys %s against %s" % (sorted(got), sorted(want)))
    for k in sorted(got):
        d = difference(k, got[k], want[k], body)
        if d is not None:
            return (k,) + d
    return None


# ---- sequences ----------------------------------------------------------------------------------------------------------------
def euler_circuit(names):
    """a closed walk over `names` in which every ordered pair (a, b), a == b included, is consecutive exactly once: an Eulerian
    circuit of the complete digraph with loops (Hierholzer), len(names)^2 + 1 steps"""
    names = list(names)
    nxt = {a: list(reversed(names)) for a in names}
    stack, walk = [names[0]], []
    while stack:
        a = stack[-1]
        if nxt[a]:
            stack.append(nxt[a].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == len(names) ** 2 + 1
    return walk


def pairs_of(seq):
    return {(a, b) for a, b in zip(seq[:-1], seq[1:])}
