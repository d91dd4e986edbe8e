"""test.py:18-23's `lpips.LPIPS(net='alex' | 'vgg')` on the device (include/dsnerf.h "LPIPS", csrc/dsn_lpips.hip).

    loss_fn_alex = dsnerf_amd.lpips.LPIPS(net="alex", state_dict=sd).to(device)      # the one-line swap
    lpips_alex = loss_fn_alex(pred, gt)          # NCHW RGB in [-1, 1] -> [N,1,1,1] float32 on the device; float64 in .last

The weights come from the caller (this package downloads nothing): either the package's own `LPIPS.state_dict()`, or the pair
(torchvision `features` state dict, the package's lin file).  Parity with the `lpips` package is unverified where this was written
(neither lpips nor torchvision was available): the kernels are pinned to a restatement of the rule in include/dsnerf.h
(tests/lpips_restate.py); tests/test_lpips_package.py compares with the package wherever it imports.
"""
from __future__ import annotations

import torch

from . import _lib

# torchvision `features` indices of the convolutions, in layer order
FEATURE_INDEX = {"alex": (0, 3, 6, 8, 10), "vgg": (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)}
# the package's slices: slice K of net.sliceK holds the features up to tap K
_SLICE_END = {"alex": (2, 5, 8, 10, 12), "vgg": (4, 9, 16, 23, 30)}


def _slice_of(net, index):
    for k, end in enumerate(_SLICE_END[net]):
        if index < end:
            return k + 1
    raise AssertionError(index)


def _take(sd, key):
    if key not in sd:
        raise KeyError(f"LPIPS weights: tensor '{key}' is missing")
    return torch.as_tensor(sd[key]).detach()


def weights_from_package(net, state_dict):
    """(conv, lin) from the package's own LPIPS.state_dict(): net.sliceK.<features index>.weight | bias and linK.model.1.weight
    (K = 0 .. 4); the duplicated lins.K.model.1.weight keys and the scaling layer's buffers are ignored"""
    conv = [(_take(state_dict, f"net.slice{_slice_of(net, i)}.{i}.weight"), _take(state_dict, f"net.slice{_slice_of(net, i)}.{i}.bias"))
            for i in FEATURE_INDEX[net]]
    lin = [_take(state_dict, f"lin{k}.model.1.weight") for k in range(5)]
    return conv, lin


def weights_from_pair(net, features_sd, lin_sd):
    """(conv, lin) from torchvision's state dict (features.N.weight | bias; keys without the `features.` prefix are accepted) and the
    package's lin file (linK.model.1.weight)"""
    pre = "features." if any(k.startswith("features.") for k in features_sd) else ""
    conv = [(_take(features_sd, f"{pre}{i}.weight"), _take(features_sd, f"{pre}{i}.bias")) for i in FEATURE_INDEX[net]]
    lin = [_take(lin_sd, f"lin{k}.model.1.weight") for k in range(5)]
    return conv, lin


def load_weights(net, state_dict):
    """the canonical lists (conv = [(weight, bias)] in layer order, lin = five vectors) from either layout; shapes checked, a missing
    or mis-shaped tensor is named"""
    if net not in _lib.LPIPS_NETS:
        raise ValueError(f"net must be 'alex' or 'vgg', got {net!r}")
    if isinstance(state_dict, (tuple, list)) and len(state_dict) == 2 and all(hasattr(d, "keys") for d in state_dict):
        conv, lin = weights_from_pair(net, *state_dict)
    elif hasattr(state_dict, "keys"):
        conv, lin = weights_from_package(net, state_dict)
    else:
        raise TypeError("state_dict must be the package's LPIPS.state_dict() or a pair (features state dict, lin state dict)")
    for (w, b), i, sh in zip(conv, FEATURE_INDEX[net], _lib.LPIPS_CONV_SHAPES[net]):
        if tuple(w.shape) != sh:
            raise ValueError(f"LPIPS weights: features {i} weight must be {sh}, got {tuple(w.shape)}")
        if tuple(b.shape) != (sh[0],):
            raise ValueError(f"LPIPS weights: features {i} bias must be {(sh[0],)}, got {tuple(b.shape)}")
    lin = list(lin)
    for k, c in enumerate(_lib.LPIPS_TAP_CHANNELS[net]):
        if tuple(lin[k].shape) not in ((1, c, 1, 1), (c,)):
            raise ValueError(f"LPIPS weights: lin{k}.model.1.weight must be {(1, c, 1, 1)}, got {tuple(lin[k].shape)}")
        lin[k] = lin[k].reshape(-1)
    return conv, lin


class LPIPS:
    """Callable like the package's object: loss_fn(pred, gt) with NCHW RGB tensors in [-1, 1] (normalize=True: in [0, 1]) returns a
    [N,1,1,1] float32 device tensor; the float64 values, per-tap terms and status words of the last call are in .last, .last_layers
    and .last_status (device tensors: nothing is synchronised).  A frame with a status is NaN (_lib.lpips_status_text)."""

    def __init__(self, net="alex", state_dict=None, device=None):
        if state_dict is None:
            raise ValueError("LPIPS: state_dict is required (the package's LPIPS.state_dict(), or (features state dict, lin state dict))")
        self.net = net
        self.conv, self.lin = load_weights(net, state_dict)
        self.device = None
        self.packed = None
        self.last = self.last_layers = self.last_status = None
        if device is not None:
            self.to(device)

    def to(self, device):
        device = torch.device(device)
        if self.packed is None or device != self.device:
            self.packed = _lib.lpips_pack(self.net, self.conv, self.lin, device)
            self.device = device
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    def eval(self):
        return self

    def distance(self, img, gt, rgb_pm1=False):
        """the library's own surface: [F,H,W,3] stacks (BGR in [0,1] unless rgb_pm1) -> (out float64 [F], layers [F,5], status [F])"""
        if self.packed is None:
            self.to(img.device)
        return _lib.lpips(self.net, self.packed, img, gt, rgb_pm1=rgb_pm1)

    def __call__(self, in0, in1, normalize=False):
        if in0.dim() != 4 or in0.shape[1] != 3 or in0.shape != in1.shape:
            raise ValueError(f"LPIPS: two [N,3,H,W] tensors expected, got {tuple(in0.shape)} and {tuple(in1.shape)}")
        if self.packed is None:
            self.to(in0.device)
        a = in0.to(device=self.device, dtype=torch.float32)
        b = in1.to(device=self.device, dtype=torch.float32)
        if normalize:
            a, b = 2.0 * a - 1.0, 2.0 * b - 1.0
        a = a.permute(0, 2, 3, 1).contiguous()
        b = b.permute(0, 2, 3, 1).contiguous()
        self.last, self.last_layers, self.last_status = _lib.lpips(self.net, self.packed, a, b, rgb_pm1=True)
        return self.last.to(torch.float32).reshape(-1, 1, 1, 1)

    forward = __call__
