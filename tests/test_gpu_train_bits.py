"""The training backward's trunk gradients against RECORDED bits (tests/golden/train_grad_bits.json).

test_gpu_train.py and test_gpu_train_rows.py judge every parameter gradient against float64 with a tolerance; a refactor of
dsn_train_run must not move one bit of what the default step computes, and a tolerance cannot see that.  The trunk's weight and bias
gradients (every parameter whose name contains `stage`) come out of the two-stage split-fp16 products, whose summation order is fixed:
they are the same bits from process to process (test_gpu_round5.py::test_paired_weight_gradient_launches_match_the_single_ones holds
that for one case).  The fixture holds, per case and per such tensor, the SHA-256 of the gradient's raw float32 bytes, its float64 sum
and its L2 norm.  Tensors outside the trunk end in float atomics and stay with the float64 oracles of the two modules above.

The cases are the smallest golden gradient cases that reach each dispatch of the step:
  small_train_grads_w4        fewer than 4096 rows: one stream
  full_train_grads_w4         128 x 64 = 8192 rows: two streams, the compositing adjoint's wave form <1>
  full_train_grads_w4_s128    the wave form <2> (65 <= S <= 128)
  full_train_grads_s200       the one-thread-per-ray adjoint above S = 128

The fixture was recorded with scripts/record_train_bits.py from the library of the commit BEFORE the one that added this module (the
recorder takes the library's path), each case in two child processes with the default environment (tests/_grads_dump.py); the
recorder refuses to write unless the two processes agree bit for bit on every trunk tensor of every case - all four cases did.  It is
never re-recorded from the build under test: a change that moves a trunk bit on purpose re-records from its own parent's point of
view, i.e. says so in its diff."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from row_cotangents import load_case
from test_gpu_render import make_batch, make_renderer
from test_gpu_train import reference_loss

pytestmark = pytest.mark.gpu

CASES = ("small_train_grads_w4", "full_train_grads_w4", "full_train_grads_w4_s128", "full_train_grads_s200")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_grad_bits.json")


def digest(a):
    """what the fixture holds of one gradient tensor"""
    a = np.ascontiguousarray(a, dtype="<f4")
    d = a.astype(np.float64)
    return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "sum": float(d.sum()), "norm": float(np.sqrt((d * d).sum())),
            "shape": list(a.shape)}


def trunk_digests(grads):
    """{name: digest} of the trunk tensors of {name: gradient array}"""
    return {k: digest(a) for k, a in sorted(grads.items()) if "stage" in k}


def gradients(name):
    """one training forward + backward of a golden case in this process, as tests/_grads_dump.py runs it"""
    g = load_case(name)
    r = make_renderer(g, name)
    r.cfg.MODEL.raw_noise_std = float(g["raw_noise_std"])
    r.train()
    torch.manual_seed(int(g["seed"]))
    out = r.render(make_batch(g))["coarse"]
    loss = reference_loss(out, torch.from_numpy(g["target_rgb"]).cuda(), torch.from_numpy(g["occupancy"]).cuda())
    r.net.zero_grad()
    loss.backward()
    return {k: p.grad.detach().cpu().numpy() for k, p in r.net.named_parameters()}


@pytest.fixture(scope="module")
def want():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("name", CASES)
def test_trunk_gradient_bits(want, name):
    rec, got = want[name], trunk_digests(gradients(name))
    assert sorted(got) == sorted(rec) and len(rec) == 14,(sorted(got), sorted(rec))
    assert all(np.isfinite(v["norm"]) and v["norm"] > 0 for v in rec.values()), "the recorded trunk gradients are not zero"
    bad = [k for k in rec if got[k]["sha256"] != rec[k]["sha256"] or got[k]["shape"] != rec[k]["shape"]]
    for k in bad:
        print("%s %s: recorded sum %.17g norm %.17g, now sum %.17g norm %.17g" % (name, k, rec[k]["sum"], rec[k]["norm"], got[k]["sum"], got[k]["norm"]))
    assert not bad, "%d of %d trunk gradients differ from the recorded bits: %r" % (len(bad), len(rec), bad)
