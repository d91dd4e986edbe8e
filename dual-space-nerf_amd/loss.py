"""utils/loss.py on the device: make_loss(cfg), MSELoss(cfg), SmoothL1Loss(cfg) with the reference's names and call.

    loss_fn = make_loss(cfg)
    loss1 = loss_fn(coarse, batch)            # {"loss_rgb": ...} (+ "loss_mask" with cfg.MODEL.LOSSwMask), trainer.py:70-81 unchanged
    psnr = loss_fn.last["psnr"]               # the trainer's psnr(coarse["color"], batch["rgb"]) of the same call, no extra launch

One forward launch pair (dsn_train_loss: both losses, mse and psnr in fp64, the reference's acc_map[occupancy == 1] = 1 in the same
pass) and one backward launch (dsn_train_loss_grad: the seeds of color and acc_map, scaled by the upstream gradients read on the
device) behind ONE autograd node; the rule is in include/dsnerf.h.  Nothing synchronises until the caller reads a value.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib


class _TrainLoss(torch.autograd.Function):
    """(color, acc_map) -> (loss_rgb, loss_mask[, acc_map]): acc_map comes back, marked dirty, when the kernel overwrote it"""

    @staticmethod
    def forward(ctx, color, acc, target, occupancy, kind, overwrite, owner):
        mask_on = occupancy is not None
        res = _lib.train_loss(color, target, acc if mask_on else None, occupancy, kind=kind, overwrite_acc=overwrite,
                              workspace=owner._ws)
        owner._ws = res["workspace"]
        owner.last = {k: res[k] for k in ("mse", "psnr", "loss_rgb", "loss_mask")}
        ctx.kind, ctx.mask_on = kind, mask_on
        ctx.dirty = bool(mask_on and overwrite)
        ctx.target, ctx.occupancy = target, occupancy          # data: no gradient, not part of the graph
        ctx.set_materialize_grads(False)
        # (views of their own: `last` keeps tensors without a graph, the outputs get autograd's bookkeeping; no launch)
        loss_rgb, loss_mask = res["losses_f32"][0], res["losses_f32"][1]
        if ctx.dirty:
            ctx.mark_dirty(acc)
            ctx.save_for_backward(color, acc)
            return loss_rgb, loss_mask, acc
        ctx.save_for_backward(color, acc if mask_on else None)
        return loss_rgb, loss_mask

    @staticmethod
    def backward(ctx, up_rgb, up_mask, g_acc_out=None):
        color, acc = ctx.saved_tensors
        g_color, g_acc = _lib.train_loss_grad(color, ctx.target, acc, ctx.occupancy, kind=ctx.kind, up_rgb=up_rgb, up_mask=up_mask,
                                              want_acc=ctx.mask_on and ctx.needs_input_grad[1])
        if g_acc_out is not None and ctx.needs_input_grad[1]:      # acc_map used again after the call: rays set to 1 pass nothing on
            g_acc = g_acc + g_acc_out.reshape(-1).masked_fill(ctx.occupancy.reshape(-1).to(g_acc.device) == 1, 0.0)
        return (g_color.reshape(color.shape) if ctx.needs_input_grad[0] else None,
                g_acc.reshape(acc.shape) if g_acc is not None else None, None, None, None, None, None)


class _DeviceLoss(nn.Module):
    KIND = None

    def __init__(self, cfg, overwrite_acc=True):
        super().__init__()
        self.cfg = cfg
        self.overwrite_acc = bool(overwrite_acc)
        self.last = {}           # {"mse", "psnr" (float64), "loss_rgb", "loss_mask" (float32)} of the latest call, device tensors
        self._ws = None

    def forward(self, inputs, batch, overwrite_acc=None):
        color = inputs["color"]
        dev = color.device
        target = batch["rgb"].reshape(-1, 3).to(dev)                     # (the reference: .cuda())
        with_mask = bool(self.cfg.MODEL.LOSSwMask)
        acc = inputs["acc_map"] if with_mask else None
        occupancy = batch["occupancy"].reshape(-1).to(dev) if with_mask else None
        overwrite = self.overwrite_acc if overwrite_acc is None else bool(overwrite_acc)
        out = _TrainLoss.apply(color, acc, target, occupancy, self.KIND, overwrite, self)
        ret = {"loss_rgb": out[0]}
        if with_mask:
            ret["loss_mask"] = out[1]
        return ret


class MSELoss(_DeviceLoss):
    """utils/loss.py:11-29"""
    KIND = "L2"


class SmoothL1Loss(_DeviceLoss):
    """utils/loss.py:31-49 (nn.SmoothL1Loss: beta = 1)"""
    KIND = "L1"


def make_loss(cfg, overwrite_acc=True):
    """utils/loss.py:4-8.  An unknown cfg.MODEL.LOSS raises (the reference returns None and fails at the first call)."""
    if cfg.MODEL.LOSS == "L2":
        return MSELoss(cfg, overwrite_acc)
    if cfg.MODEL.LOSS == "L1":
        return SmoothL1Loss(cfg, overwrite_acc)
    raise ValueError(f"cfg.MODEL.LOSS must be 'L2' or 'L1', got {cfg.MODEL.LOSS!r}")
