"""The body model on the device: SMPL parameters -> posed vertices, joint transforms and bounds for a whole clip (dsn_body_shape /
dsn_body_pose, the rule of include/dsnerf.h).

The reference reads the posed vertices from new_vertices/{i}.npy (tool/generate_novelpose_vertices.py writes them off-line through
EasyMocap's SMPL layer, per performer) and the Human3.6M datasets run utils/h36m_utils.get_rigid_transformation / get_bounds per item.
BodyModel holds the model's arrays on the device in the kernels' layouts and makes batch["xyz"], the datasets' pxyz, the joint transforms
of lbs_warp and the bounds of camera_rays for P poses per library call.  24 joints; hands and face models are out of scope, and so are
the SMPL pickle's chumpy objects (hand over plain arrays: np.asarray(obj.r) where the pickle holds chumpy)."""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib

N_JOINTS, N_POSE_FEATURES = 24, 207


def _dense(a):
    """a dense float32 numpy array of anything array-like, scipy.sparse matrices included"""
    if hasattr(a, "toarray"):
        a = a.toarray()
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


class BodyModel:
    """v_template [V,3], weights [V,24], parents [24] (or a kintree_table [2,24]: its first row); J_regressor [24,V] (dense or
    scipy.sparse) or joints [24,3] (one of the two; joints given directly are kept until set_shape recomputes them from a regressor);
    shapedirs [V,3,B]; posedirs in the pickle's layout [V,3,207] or the kernel's [207,3V].  Everything is kept as float32 tensors on
    `device` (default: the current ROCm device; "cpu" holds the layouts only - pose() and set_shape() need the GPU)."""

    def __init__(self, v_template, weights, parents, J_regressor=None, joints=None, shapedirs=None, posedirs=None, device=None):
        if device is None:
            _lib.require_gpu()
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        up = lambda a: torch.from_numpy(a).to(self.device)      # noqa: E731
        vt = _dense(v_template).reshape(-1, 3)
        self.V = V = vt.shape[0]
        if V < 1:
            raise ValueError("BodyModel: no vertices")
        w = _dense(weights)
        if w.shape != (V, N_JOINTS):
            raise ValueError(f"BodyModel: weights must be [{V},{N_JOINTS}], got {w.shape}")
        par = np.asarray(parents.detach().cpu().numpy() if torch.is_tensor(parents) else parents)
        if par.ndim == 2:                      # kintree_table: row 0 holds the parents (row 1 the joint ids)
            par = par[0]
        par = par.astype(np.int64).reshape(-1)
        if par.shape[0] != N_JOINTS:
            raise ValueError(f"BodyModel: {par.shape[0]} parents, the library's body has {N_JOINTS} joints")
        par = par.copy()
        par[0] = -1                            # (the pickle stores 2^32 - 1 there)
        if any(not (0 <= par[i] < i) for i in range(1, N_JOINTS)):
            raise ValueError("BodyModel: parents[i] must be an earlier joint (0 <= parents[i] < i) for every i >= 1")
        self.parents = par.astype(np.int32)
        self._parents_c = _lib.body_parents(self.parents)
        self.v_template, self.weights = up(vt), up(w)
        self.J_regressor = self.shapedirs = self.posedirs = None
        if J_regressor is not None:
            Jr = _dense(J_regressor)
            if Jr.shape != (N_JOINTS, V):
                raise ValueError(f"BodyModel: J_regressor must be [{N_JOINTS},{V}], got {Jr.shape}")
            self.J_regressor = up(Jr)
        if shapedirs is not None:
            sd = _dense(shapedirs)
            if sd.ndim != 3 or sd.shape[:2] != (V, 3):
                raise ValueError(f"BodyModel: shapedirs must be [{V},3,B], got {sd.shape}")
            self.shapedirs = up(sd)
        if posedirs is not None:
            pd = _dense(posedirs)
            if pd.shape == (V, 3, N_POSE_FEATURES):
                pd = np.ascontiguousarray(pd.reshape(3 * V, N_POSE_FEATURES).T)
            elif pd.shape != (N_POSE_FEATURES, 3 * V):
                raise ValueError(f"BodyModel: posedirs must be [{V},3,{N_POSE_FEATURES}] or [{N_POSE_FEATURES},{3 * V}], got {pd.shape}")
            self.posedirs = up(pd)
        self.v_shaped = self.v_template
        self.joints = None
        if joints is not None:
            j = _dense(joints).reshape(-1, 3)
            if j.shape[0] != N_JOINTS:
                raise ValueError(f"BodyModel: joints must be [{N_JOINTS},3], got {j.shape}")
            self.joints = up(j)
        elif self.J_regressor is None:
            raise ValueError("BodyModel: give J_regressor or joints")
        elif self.device.type == "cuda":
            self.set_shape(None)
        self._ws = None

    @classmethod
    def from_smpl_dict(cls, data, device=None):
        """from the unpickled SMPL model (can_render.load_bodydata): v_template, weights, kintree_table, J_regressor (scipy.sparse),
        shapedirs [V,3,B], posedirs [V,3,207]"""
        return cls(data["v_template"], data["weights"], data["kintree_table"], J_regressor=data.get("J_regressor"),
                   shapedirs=data.get("shapedirs"), posedirs=data.get("posedirs"), device=device)

    @classmethod
    def from_lbs_dir(cls, arrays, device=None):
        """from the datasets' lbs/ arrays: a dict (or the directory's path) with joints [24,3], parents [24], weights [V,24] and the
        canonical vertices "tvertices" [V,3] - what h36m_dataset.py hands get_rigid_transformation; no pose or shape blend shapes"""
        if isinstance(arrays, (str, os.PathLike)):
            arrays = {k: np.load(os.path.join(arrays, k + ".npy")) for k in ("joints", "parents", "weights", "tvertices")}
        return cls(arrays["tvertices"], arrays["weights"], arrays["parents"], joints=arrays["joints"], device=device)

    def set_shape(self, betas=None):
        """dsn_body_shape: v_shaped = v_template + shapedirs . betas (None: the template) and, with a regressor, the joints of that
        shape.  Returns self."""
        if betas is not None and self.shapedirs is None:
            raise ValueError("BodyModel.set_shape: the model has no shapedirs")
        sd = None
        if betas is not None:
            betas = torch.as_tensor(betas, dtype=torch.float32).reshape(-1).to(self.device)
            B = betas.shape[0]
            if B > self.shapedirs.shape[2]:
                raise ValueError(f"BodyModel.set_shape: {B} betas, the model has {self.shapedirs.shape[2]} shape directions")
            sd = self.shapedirs if B == self.shapedirs.shape[2] else self.shapedirs[:, :, :B].contiguous()
        self.v_shaped, joints = _lib.body_shape(self.v_template, sd, betas, self.J_regressor)
        if joints is not None:
            self.joints = joints
        return self

    def slab_poses(self, budget_bytes=256 << 20):
        """poses per library call: as many as keep workspace + outputs of one call within budget_bytes"""
        per_pose = 4 * (2 * 3 * self.V + 16 * N_JOINTS + 6 + 9) + (_lib.lib().dsn_body_pose_workspace_bytes(self.V, 64) + 63) // 64
        return int(max(1, min(1 << 18, budget_bytes // per_pose)))

    @torch.no_grad()
    def pose(self, poses, Rh=None, Th=None, pad=None, want=("xyz", "A", "bounds"), slab=None):
        """poses [P,24,3] (or [P,72]), Rh / Th [P,3] or None (identity / zero), pad: None, "zju_train", "zju_eval" or "h36m" ->
        {"xyz" [P,V,3] world vertices, "A" [P,24,4,4] (lbs_warp's joint_transforms), "bounds" [P,2,3], and on request "xyz_smpl"
        [P,V,3] (before Rh / Th: the datasets' pxyz) and "Rh_mat" [P,3,3]}: device tensors.  One library call per `slab` poses
        (default: slab_poses()); the bits do not depend on it."""
        _lib.require_gpu()
        if self.joints is None:
            raise RuntimeError("BodyModel.pose: no joints (set_shape first)")
        dev = self.device
        f = lambda t, n: None if t is None else torch.as_tensor(t).to(device=dev, dtype=torch.float32).reshape(-1, *n).contiguous()      # noqa: E731
        poses, Rh, Th = f(poses, (N_JOINTS, 3)), f(Rh, (3,)), f(Th, (3,))
        P = poses.shape[0]
        slab = self.slab_poses() if slab is None else max(1, int(slab))
        call = lambda a, b: _lib.body_pose(self.v_shaped, self.joints, self._parents_c, self.weights, self.posedirs, poses[a:b],      # noqa: E731
                                           None if Rh is None else Rh[a:b], None if Th is None else Th[a:b], pad, want, self._ws)
        if P <= slab:
            return call(0, P)
        nbytes = _lib.lib().dsn_body_pose_workspace_bytes(self.V, slab)
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = _lib._scratch(nbytes, dev)
        parts = [call(a, min(a + slab, P)) for a in range(0, P, slab)]
        return {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]}
