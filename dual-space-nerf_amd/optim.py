"""solver/build.py on the device: make_optimizer(cfg, model) with the reference's signature, and the optimizer it builds.

    optimizer = make_optimizer(cfg, model)          # main.py:107, trainer.py:66-81 unchanged
    scheduler = build_scheduler(optimizer, ...)      # solver/lr_scheduler.py:58-71 unchanged (LambdaLR writes group["lr"])

Adam is torch.optim.Adam's default algorithm (L2 weight decay, no amsgrad) with the state layout of torch.optim.Adam - state_dict()
and load_state_dict() go both ways between the two classes, so utils/checkpoint.py's Checkpointer saves and resumes it - and ONE
launch per step for all tensors (dsn_adam_step; the rule is in include/dsnerf.h, float32 without fused multiply-add, restated bit for
bit by tests/adam_restate.py).  With net= the same call leaves the model's packed image current behind the update, so the next
render's net.packed() has nothing to compare-and-repack.  step() makes no device-to-host copy and never synchronises.
"""
from __future__ import annotations

import weakref

import torch

from . import _lib

_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable", "fused", "foreach", "decoupled_weight_decay")
# torch.optim.Adam's own values for them: the param groups carry the same keys, so a state_dict loads into either class
_TORCH_GROUP_DEFAULTS = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                             decoupled_weight_decay=False)


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay) in one launch per step.

    params: an iterable of parameters or a list of param-group dicts; every parameter a contiguous float32 tensor on a GPU
    (ValueError otherwise: nothing falls back to another arithmetic).  amsgrad, maximize, capturable, differentiable, fused, foreach,
    decoupled_weight_decay and sparse gradients are not implemented: ValueError naming the keyword.
    net: the DualSpaceNeRF whose packed image the step keeps current (held weakly; bind()).  Honoured when the optimizer holds all 33
    of its parameters on one GPU and those with a gradient share one step count and one set of betas and eps; otherwise the
    parameters are updated and the image is left to net.packed(), which sees the advanced version counters and re-packs.  Parameters
    of the optimizer that are not the net's are updated by calls of their own either way."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, net=None, **unsupported):
        for k, v in unsupported.items():
            if k not in _UNSUPPORTED:
                raise TypeError(f"Adam() got an unexpected keyword argument {k!r}")
            if v:
                raise ValueError(f"dsnerf_amd.optim.Adam does not implement {k}={v!r}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **_TORCH_GROUP_DEFAULTS)
        _check_group(defaults)
        super().__init__(params, defaults)
        self._net = None             # weak: the optimizer holds the 33 tensors, not the module
        self._net_params = None
        if net is not None:
            self.bind(net)

    def bind(self, net):
        """name the DualSpaceNeRF whose packed image step() keeps current (what net= does at construction; a copied or unpickled
        optimizer carries no binding and is bound again with this).  Evaluated again whenever a param group is added."""
        named = dict(net.named_parameters())
        mine = {id(p) for g in self.param_groups for p in g["params"]}
        tensors = [named.get(k) for k in _lib.PARAM_ORDER]
        self._net = weakref.ref(net)
        self._net_params = None
        if all(t is not None and id(t) in mine for t in tensors) and len({t.device for t in tensors}) == 1:
            self._net_params = tensors

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("_net", None)
        self.__dict__.setdefault("_net_params", None)

    def add_param_group(self, param_group):
        params = param_group["params"]
        for p in ([params] if isinstance(params, torch.Tensor) else list(params)):
            if not isinstance(p, torch.Tensor):
                continue          # (torch's own TypeError follows)
            if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous() or p.is_sparse:
                raise ValueError("dsnerf_amd.optim.Adam updates contiguous float32 tensors on a GPU: got "
                                 f"{p.dtype} {tuple(p.shape)} on {p.device} (contiguous: {p.is_contiguous()})")
        super().add_param_group(param_group)
        _check_group(self.param_groups[-1])
        net = self.__dict__.get("_net")
        if net is not None and net() is not None:
            self.bind(net())

    def load_state_dict(self, state_dict):
        for group in state_dict["param_groups"]:          # (before anything of it is taken over)
            _check_flags(group)
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            _check_group(group)
        for st in self.state.values():          # a capturable / fused torch Adam keeps `step` on the device: here it lives on the host
            if "step" in st and (st["step"].is_cuda or st["step"].dtype != torch.float32):
                st["step"] = st["step"].detach().to(device="cpu", dtype=torch.float32)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # every group and gradient is looked at before anything changes: a refusal leaves no step count advanced
        work = []
        for group in self.param_groups:
            _check_group(group)
            lr, wd = float(group["lr"]), float(group["weight_decay"])
            hyper = (float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]))
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise ValueError("dsnerf_amd.optim.Adam does not implement sparse gradients")
                if g.dtype != torch.float32 or g.device != p.device:
                    raise ValueError(f"a gradient must be float32 on its parameter's device, got {g.dtype} on {g.device}")
                work.append((p, g, lr, wd, hyper))
        if not work:
            return loss
        calls = {}           # (beta1, beta2, eps, t, device) -> {id(p): (p, grad, exp_avg, exp_avg_sq, lr, weight_decay)}
        for p, g, lr, wd, hyper in work:
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["step"] += 1
            calls.setdefault(hyper + (float(st["step"]), p.device), {})[id(p)] = (p, g.contiguous(), st["exp_avg"], st["exp_avg_sq"], lr, wd)
        # the net's 33 tensors in one call that rebuilds the image behind them; every other tensor of the optimizer in calls of its own
        packed, key = self._packed_for(calls)
        if packed is not None:
            rows = calls[key]
            self._launch(key, [rows.pop(id(p), (p, None, None, None, 0.0, 0.0)) for p in self._net_params], packed)
        for key, rows in calls.items():
            if rows:
                self._launch(key, list(rows.values()), None)
        # the storage changed under the tensors: what an in-place op does to the version counters (_RenderRays' saved parameters
        # raise in backward after a step; net.packed() re-packs unless told below that the image is current)
        torch.autograd.graph.increment_version([w[0] for w in work])
        if packed is not None:
            packed.note_repacked(self._net_params)
        return loss

    def _packed_for(self, calls):
        """(the net's PackedParams, the key of the call its tensors are in) when this step may rebuild the image, else (None, None):
        the binding holds, the net's tensors are where they were, and those with a gradient share one call"""
        tensors = self._net_params
        net = self._net() if self._net is not None else None
        if tensors is None or net is None:
            return None, None
        ids = {id(t) for t in tensors}
        keys = [key for key, rows in calls.items() if not ids.isdisjoint(rows)]
        dev = tensors[0].device
        if len(keys) != 1 or any(t.device != dev or not t.is_contiguous() for t in tensors):
            return None, None
        if net._packed is None:
            net._packed = _lib.PackedParams(dev)
        return (net._packed, keys[0]) if net._packed.device == dev else (None, None)

    @staticmethod
    def _launch(key, rows, packed):
        b1, b2, eps, t, _ = key
        p, g, m, v, lr, wd = zip(*rows)
        # (a tensor without a gradient: its moments are not looked at)
        m = [p[i] if x is None else x for i, x in enumerate(m)]
        v = [p[i] if x is None else x for i, x in enumerate(v)]
        _lib.adam_step(list(p), list(g), m, v, lr, wd, (b1, b2), eps, t, packed=packed)


def _check_flags(group):
    for k in _UNSUPPORTED:
        if group.get(k):
            raise ValueError(f"dsnerf_amd.optim.Adam does not implement {k}={group[k]!r}")


def _check_group(group):
    _check_flags(group)
    lr, eps, wd = group["lr"], group["eps"], group["weight_decay"]
    for name, x in (("lr", lr), ("eps", eps), ("weight_decay", wd)):
        if isinstance(x, torch.Tensor) and x.is_cuda:
            raise ValueError(f"{name} as a device tensor would make step() synchronise: pass a number")
        if not 0.0 <= float(x):
            raise ValueError(f"Invalid {name}: {x}")
    for i, b in enumerate(group["betas"]):
        if isinstance(b, torch.Tensor) and b.is_cuda:
            raise ValueError("betas as device tensors would make step() synchronise: pass numbers")
        if not 0.0 <= float(b) < 1.0:
            raise ValueError(f"Invalid beta parameter at index {i}: {b}")


def make_optimizer(cfg, model, active_list=[], frozen_list=[]):
    """solver/build.py:3-19: Adam over model.parameters(), or the frozen (lr 0) / active two-group form.  A DualSpaceNeRF `model`
    is handed on as net=.  Another cfg.SOLVER.OPTIMIZER_NAME raises (the reference falls through to an unbound name)."""
    from .model.spacenet import DualSpaceNeRF
    weight_decay = cfg.SOLVER.WEIGHT_DECAY
    lr = cfg.SOLVER.BASE_LR
    if cfg.SOLVER.OPTIMIZER_NAME != "Adam":
        raise ValueError(f"cfg.SOLVER.OPTIMIZER_NAME must be 'Adam', got {cfg.SOLVER.OPTIMIZER_NAME!r}")
    net = model if isinstance(model, DualSpaceNeRF) else None
    if active_list == [] and frozen_list == []:
        return Adam(params=model.parameters(), lr=lr, betas=(0.9, 0.999), weight_decay=weight_decay, net=net)
    return Adam([{"params": frozen_list, "lr": 0.0},
                 {"params": active_list, "lr": lr}], lr=lr, betas=(0.9, 0.999), weight_decay=weight_decay, net=net)
