"""TEST INFRASTRUCTURE: the two networks of the hot path restated in float64 torch at arbitrary points (the role maps_restate.py and
mc_restate.py play for their features) - what tests/test_gpu_tiles.py judges k_field16 / k_field / k_light16 / k_light by.

field64: model/spacenet.py:93-148 (+ :223-236 pose code, :125-129 frame code, :301-311 d sigma/dx), laid out as
oracle/train_oracle.py's render does it, WITHOUT that function's geometry and compositing: the canonical points are an argument.
light64: model/spacenet.py:174-188 LightingMLP on [n_w, x_w, view_dir] (no light-centre / rotation edit: those move x_w before the MLP,
model/spacenet.py:254-265, and belong to the caller).

Every input is the float32 value a kernel receives, cast up; every weight is the checkpoint's float32 value, cast up; the pose code is
the float32 pose MLP's output, cast up (the networks of the product evaluate it in float32 once per frame).  Pinned against the
reference's own float64 and float32 runs by tests/test_field_restate_host.py.
"""
import numpy as np
import torch

from train_oracle import encode, linear, rod2quat


def _params(state_dict, dtype=torch.float64):
    return {k: torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float32))).to(dtype) for k, v in state_dict.items()}


def pose_code(state_dict, poses, rows=1):
    """model/spacenet.py:223-236: the 16-value pose code of a frame in float32, as the reference and the kernels evaluate it.
    rows > 1: the MLP on the quaternion repeated `rows` times [rows,16], as the reference's forward runs it (:229-236) - torch's
    batched float32 product may round differently from its single-row one (last bits)"""
    p = _params(state_dict, torch.float32)
    q = rod2quat(torch.from_numpy(np.ascontiguousarray(np.asarray(poses, np.float32).reshape(24, 3))), torch.float32).repeat(int(rows), 1)
    return linear(p, "pose_mlp.4", torch.relu(linear(p, "pose_mlp.2", torch.relu(linear(p, "pose_mlp.0", q)))))


def field64(x, state_dict, poses, frame, zero_code=False, pose=None):
    """x [N,3] canonical points -> float64 numpy (sigma [N], essence [N,3], grad_sigma [N,3]).
    pose (optional): the pose code to use, [1,16] or [N,16], instead of pose_code(state_dict, poses)"""
    f64 = torch.float64
    p = _params(state_dict)
    x = torch.from_numpy(np.ascontiguousarray(np.asarray(x).reshape(-1, 3))).to(f64).requires_grad_(True)
    N = x.shape[0]
    pose = (pose_code(state_dict, poses) if pose is None else torch.as_tensor(pose)).to(f64).reshape(-1, 16)
    code = p["nerf.embedding.weight"][int(frame)][None]
    if zero_code:
        code = code * 0
    pe = encode(x)
    h = torch.cat([code.expand(N, -1), pe, pose.expand(N, -1)], dim=-1)
    for k in (0, 2, 4, 6):
        h = torch.relu(linear(p, f"nerf.stage1.{k}", h))
    h = torch.cat([h, pe], dim=-1)
    for k in (0, 2, 4):
        h = torch.relu(linear(p, f"nerf.stage2.{k}", h))
    sigma = linear(p, "nerf.density_net.0", h)
    essence = linear(p, "nerf.rgb_net.3", torch.relu(linear(p, "nerf.rgb_net.1", torch.relu(h))))
    grad = torch.autograd.grad(sigma.sum(), x)[0]
    return sigma.detach().reshape(-1).numpy(), essence.detach().numpy(), grad.numpy()


def light64(n_w, x_w, view_dir, essence, state_dict):
    """[N,3] x 4 -> float64 numpy (colour [N,3] = (ELU(lighting MLP) + 1) * essence, factor [N] = ELU + 1).  view_dir is used as given
    (the kernels normalise a ray direction themselves: hand over the unit vector)."""
    f64 = torch.float64
    p = _params(state_dict)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).reshape(-1, 3))).to(f64)       # noqa: E731
    h = torch.cat([t(n_w), t(x_w), t(view_dir)], dim=-1)
    h = torch.relu(linear(p, "lighting_mlp.lights_encoding.0", h))
    h = torch.relu(linear(p, "lighting_mlp.lights_encoding.2", h))
    factor = torch.nn.functional.elu(linear(p, "lighting_mlp.lights_encoding.4", h)) + 1
    return (factor * t(essence)).numpy(), factor.reshape(-1).numpy()
