"""Golden vectors for the device loss (dsn_train_loss / dsn_train_loss_grad), from the reference's own utils/loss.py: MSELoss and
SmoothL1Loss, with and without LOSSwMask, and their total.backward() as trainer.py:70-81 runs it.  Tensor.cuda is the identity for the
duration (the classes call .cuda() on the batch); everything else is the reference's code under this container's torch.
Per case the file keeps the reference's float32 (float64 with a float64 target) losses, color.grad, acc.grad (not with a float64
target: the backward of torch's loss raises on the mixed dtypes there, has_grad says so), the acc_map it mutated, and how far its losses lie from the float64 restatement (tests/train_loss_restate.py): the bar of the tests that compare with it.
Run in the build container:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_train_loss.py"""
import os, sys
from types import SimpleNamespace
import numpy as np
import torch
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests")]
import train_loss_restate as LR  # noqa: E402

sys.path.insert(0, "/root/reference")
torch.Tensor.cuda = lambda self, *a, **k: self
from utils import loss as ref_loss  # noqa: E402

rng = np.random.RandomState(20)
out, names = {}, []
# name: R, kind, mask term, target dtype, occupancy dtype
CASES = [(R, kind, mask, "float32", "uint8") for R in (1, 63, 257) for kind in ("L2", "L1") for mask in (False, True)]
CASES += [(R, kind, True, "float64", "uint8") for R in (63, 257) for kind in ("L2", "L1")]
CASES += [(257, "L2", False, "float64", "uint8"), (257, "L1", True, "float32", "float32"), (63, "L2", True, "float64", "float32")]
CASES += [(8192, "L2", True, "float32", "uint8"), (8192, "L1", True, "float32", "uint8")]


def inputs(R):
    """one set of arrays per R: colours around the targets with a tail beyond |d| = 1 (both branches of Smooth-L1), acc in [0, 1],
    occupancy mostly 0 / 1 with a few other labels"""
    t64 = rng.rand(R, 3)
    color = (t64 + rng.randn(R, 3) * 0.6).astype(np.float32)
    acc = rng.rand(R).astype(np.float32)
    occ = (rng.rand(R) < 0.5).astype(np.uint8)
    if R > 8:
        occ[rng.permutation(R)[: max(1, R // 16)]] = 2
        acc[rng.permutation(R)[: max(1, R // 16)]] = 0.0          # acc == occ on some rays with occ == 0
    return dict(color=color, target64=t64, target32=t64.astype(np.float32), acc=acc, occ_u8=occ,
                occ_f32=np.where(occ == 2, 0.5, occ).astype(np.float32))


for R in sorted({c[0] for c in CASES}):
    for k, v in inputs(R).items():
        if R == 8192 and k == "target64":
            continue                       # (no float64-target case at this size: the file stays small)
        out[f"in{R}:{k}"] = v

for R, kind, mask, tdt, odt in CASES:
    name = f"R{R}_{kind}_{'mask' if mask else 'nomask'}_{tdt}_{odt}"
    names.append(name)
    cfg = SimpleNamespace(MODEL=SimpleNamespace(LOSS=kind, LOSSwMask=mask))
    fn = ref_loss.make_loss(cfg)
    color = torch.from_numpy(out[f"in{R}:color"].copy()).requires_grad_(True)
    acc_leaf = torch.from_numpy(out[f"in{R}:acc"].copy()).requires_grad_(True)
    acc_map = acc_leaf * 1.0                   # (the renderer's output is no leaf: the reference assigns into it in place)
    target = out[f"in{R}:target32" if tdt == "float32" else f"in{R}:target64"]
    occ = out[f"in{R}:occ_u8" if odt == "uint8" else f"in{R}:occ_f32"]
    batch = {"rgb": torch.from_numpy(target.copy())[None], "occupancy": torch.from_numpy(occ.copy())[None]}
    ret = fn({"color": color, "acc_map": acc_map}, batch)
    total = 0
    for key in ret:
        total = total + ret[key]
    try:
        total.backward()
        has_grad = True
    except RuntimeError as err:            # torch 2.10 with a float64 target: "Found dtype Double but expected Float" in the loss's backward
        assert tdt == "float64" and "Double" in str(err), err
        has_grad = False
    e = LR.forward(out[f"in{R}:color"], target, out[f"in{R}:acc"], occ if mask else None, LR.KINDS[kind])
    rec = dict(R=np.int64(R), kind=np.str_(kind), mask=np.bool_(mask), target_dtype=np.str_(tdt), occ_dtype=np.str_(odt),
               loss_rgb=ret["loss_rgb"].detach().numpy(), loss_dtype=np.str_(str(ret["loss_rgb"].dtype).replace("torch.", "")),
               has_grad=np.bool_(has_grad), acc_after=acc_map.detach().numpy())
    rec["dev_rgb"] = np.float64(abs(float(ret["loss_rgb"].detach()) - e["loss_rgb"]) / abs(e["loss_rgb"]))
    if has_grad:
        rec["color_grad"] = color.grad.numpy()
        assert color.grad.dtype == torch.float32
    if mask:
        rec.update(loss_mask=ret["loss_mask"].detach().numpy(),
                   dev_mask=np.float64(abs(float(ret["loss_mask"].detach()) - e["loss_mask"]) / abs(e["loss_mask"]) if e["loss_mask"] else 0.0))
        if has_grad:
            rec["acc_grad"] = acc_leaf.grad.numpy()
        assert ret["loss_mask"].dtype == torch.float32
        assert np.array_equal(rec["acc_after"], e["acc"])
    else:
        assert acc_leaf.grad is None and np.array_equal(rec["acc_after"], out[f"in{R}:acc"])
    if not has_grad:
        print(name, rec["loss_dtype"], "loss_rgb dev %.2e" % rec["dev_rgb"], "loss_mask dev %.2e" % rec.get("dev_mask", 0.0),
              "| the reference's backward raises with a float64 target: losses only")
        out.update({f"{name}:{k}": v for k, v in rec.items()})
        continue
    gc, ga = LR.grad(out[f"in{R}:color"], target, out[f"in{R}:acc"], occ if mask else None, LR.KINDS[kind], 1.0, 1.0)
    nz = rec["color_grad"] != 0
    print(name, rec["loss_dtype"], "loss_rgb dev %.2e" % rec["dev_rgb"], "loss_mask dev %.2e" % rec.get("dev_mask", 0.0),
          "| g_color rel %.2e" % float(np.abs(gc[nz].astype(np.float64) / rec["color_grad"][nz] - 1).max()),
          "zeros agree", bool(np.array_equal(gc == 0, ~nz)),
          "| g_acc" + (" rel %.2e, zero where occ == 1: %s" % (
              float(np.abs(ga[rec["acc_grad"] != 0].astype(np.float64) / rec["acc_grad"][rec["acc_grad"] != 0] - 1).max(initial=0.0)),
              bool((rec["acc_grad"][occ == 1] == 0).all())) if mask else " none"))
    out.update({f"{name}:{k}": v for k, v in rec.items()})
out["cases"] = np.array(names)
np.savez_compressed(os.path.join(HERE, "train_loss.npz"), **out)
print("wrote train_loss.npz", os.path.getsize(os.path.join(HERE, "train_loss.npz")), "bytes")
