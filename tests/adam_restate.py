"""TEST INFRASTRUCTURE: dsn_adam_step's rule (include/dsnerf.h) restated in numpy, one tensor at a time - float32 with one rounding
per operation (what the kernel must reproduce bit for bit), its float64 twin (the same formula with nothing rounded: the yardstick),
and the host scalars.  No torch, no library."""
import math

import numpy as np

# the model's 33 tensors in state_dict order (model/spacenet.py)
SHAPES = [(500, 8), (256, 87), (256,), (256, 256), (256,), (256, 256), (256,), (256, 256), (256,), (256, 319), (256,), (256, 256), (256,),
          (256, 256), (256,), (1, 256), (1,), (128, 256), (128,), (3, 128), (3,), (128, 9), (128,), (128, 128), (128,), (1, 128), (1,),
          (64, 92), (64,), (64, 64), (64,), (16, 64), (16,)]
TABLE, BLOCK = 48, 1024             # DSN_ADAM_TABLE, DSN_ADAM_BLOCK
U = 2.0 ** -24                      # float32's unit roundoff

f32 = np.float32


def scalars64(lr, weight_decay, betas, eps, t):
    """the rule's scalars in double, nothing rounded"""
    b1, b2 = float(betas[0]), float(betas[1])
    return dict(w1=1.0 - b1, w2=1.0 - b2, b2=b2, eps=float(eps), wd=float(weight_decay), ss=float(lr) / (1.0 - math.pow(b1, float(t))),
                c2=math.sqrt(1.0 - math.pow(b2, float(t))))


def scalars(lr, weight_decay, betas, eps, t):
    """... each rounded to float32 once"""
    return {k: f32(v) for k, v in scalars64(lr, weight_decay, betas, eps, t).items()}


def step32(p, g, m, v, s):
    """one step of one tensor: (p', m', v'), float32 arrays of p's shape.  Every line is one rounded operation."""
    p, g, m, v = (np.asarray(a, f32) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        if s["wd"] != 0:
            t = s["wd"] * p
            g = g + t
        d = g - m
        d = s["w1"] * d
        m1 = m + d
        sq = g * g
        sq = s["w2"] * sq
        v1 = s["b2"] * v
        v1 = v1 + sq
        den = np.sqrt(v1)
        den = den / s["c2"]
        den = den + s["eps"]
        q = m1 / den
        q = s["ss"] * q
        p1 = p - q
    assert p1.dtype == f32 and m1.dtype == f32 and v1.dtype == f32
    return p1, m1, v1


def step64(p, g, m, v, s):
    """the float64 twin (s: scalars64): (p', m', v', the intermediates the error bars of tests/test_adam_host.py are made of)"""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        G = np.abs(g) + s["wd"] * np.abs(p) if s["wd"] != 0 else np.abs(g)
        if s["wd"] != 0:
            g = g + s["wd"] * p
        m1 = m + s["w1"] * (g - m)
        v1 = s["b2"] * v + s["w2"] * (g * g)
        root = np.sqrt(v1)
        den = root / s["c2"] + s["eps"]
        q = m1 / den
        p1 = p - s["ss"] * q
    return p1, m1, v1, dict(G=G, root=root, den=den, q=q)


def schedule(warmup, start, end, scale=0.1):
    """the learning-rate factor of solver/lr_scheduler.py's build_scheduler as a function of the scheduler's step count k: a linear
    warm-up over `warmup` steps, 1 until `start`, then an exponential approach of `scale`"""
    def factor(k):
        k1 = k + 1.0
        if k1 <= warmup:
            return k1 / warmup
        if k1 >= start:
            return (1.0 - scale) * math.exp(-(k1 - start) / (end - start)) + scale
        return 1.0
    return factor
