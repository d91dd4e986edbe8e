"""The LPIPS rule of include/dsnerf.h restated with torch ops on the CPU (F.conv2d / F.max_pool2d), in float64 and as a float32 twin,
with the two architecture tables and hash-generated weights and images (synth.hash_uniform: the bits do not depend on the torch
version).  Test infrastructure only: the product never imports it.

`variant` switches ONE deliberate mistake on (tests/test_gpu_lpips.py::test_sensitivity_*): "no_flip", "replicate_pad", "ceil_pool",
"eps_inside", "pre_relu_taps", "alex_stride3"."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from dsnerf_amd.synth import hash_uniform  # noqa: E402

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# ("conv", Cin, Cout, k, stride, pad, tap index or None) | ("pool", k, stride)
ARCH = {
    "alex": [("conv", 3, 64, 11, 4, 2, 0), ("pool", 3, 2), ("conv", 64, 192, 5, 1, 2, 1), ("pool", 3, 2),
             ("conv", 192, 384, 3, 1, 1, 2), ("conv", 384, 256, 3, 1, 1, 3), ("conv", 256, 256, 3, 1, 1, 4)],
    "vgg": [("conv", 3, 64, 3, 1, 1, None), ("conv", 64, 64, 3, 1, 1, 0), ("pool", 2, 2),
            ("conv", 64, 128, 3, 1, 1, None), ("conv", 128, 128, 3, 1, 1, 1), ("pool", 2, 2),
            ("conv", 128, 256, 3, 1, 1, None), ("conv", 256, 256, 3, 1, 1, None), ("conv", 256, 256, 3, 1, 1, 2), ("pool", 2, 2),
            ("conv", 256, 512, 3, 1, 1, None), ("conv", 512, 512, 3, 1, 1, None), ("conv", 512, 512, 3, 1, 1, 3), ("pool", 2, 2),
            ("conv", 512, 512, 3, 1, 1, None), ("conv", 512, 512, 3, 1, 1, None), ("conv", 512, 512, 3, 1, 1, 4)],
}
TAP_CHANNELS = {"alex": (64, 192, 384, 256, 256), "vgg": (64, 128, 256, 512, 512)}
MIN_SIDE = {"alex": 31, "vgg": 16}
# torchvision `features` indices of the convolutions (the state-dict layouts of dsnerf_amd.lpips)
FEATURE_INDEX = {"alex": (0, 3, 6, 8, 10), "vgg": (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)}
# sizes of the tap tests (tests/test_gpu_lpips.py); the last three of each put a tap's pixel count at 63, 64 and 65 = one below, at and
# one above the kernel's M tile (DSN_LPIPS_TILE_M = 64): alex 31x39 -> tap 1 is 7x9, 35x35 -> 8x8, 47x111 -> tap 2 is 5x13;
# vgg 28x36 -> tap 3 is 7x9, 32x32 -> 8x8, 20x52 -> 5x13
SIZES = {"alex": [(31, 31), (35, 67), (37, 53), (64, 64), (127, 129), (128, 96), (31, 39), (35, 35), (47, 111)],
         "vgg": [(16, 16), (17, 31), (37, 53), (64, 64), (65, 63), (128, 96), (28, 36), (32, 32), (20, 52)]}
NOISE = 0.3


def conv_specs(net):
    return [op for op in ARCH[net] if op[0] == "conv"]


def make_weights(net, seed=11):
    """{"conv": [(w [Cout,Cin,k,k], b [Cout]) ...], "lin": [w [C] ...]} float32 numpy: uniform with He variance 2 / (Cin k^2),
    biases x 0.05, lin weights in [0, 1)"""
    conv, lin = [], []
    for i, (_, cin, cout, k, _, _, _) in enumerate(conv_specs(net)):
        n = cout * cin * k * k
        he = np.sqrt(2.0 / (cin * k * k))
        w = ((2.0 * hash_uniform(n, seed + 101 * i).astype(np.float64) - 1.0) * np.sqrt(3.0) * he).astype(np.float32).reshape(cout, cin, k, k)
        b = ((2.0 * hash_uniform(cout, seed + 101 * i + 50).astype(np.float64) - 1.0) * 0.05).astype(np.float32)
        conv.append((w, b))
    for l, c in enumerate(TAP_CHANNELS[net]):
        lin.append(hash_uniform(c, seed + 7000 + l).astype(np.float32))
    return {"conv": conv, "lin": lin}


def make_image(H, W, seed):
    """[H,W,3] float32 BGR in [0,1]: smooth waves plus hash texture"""
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    u = hash_uniform(H * W * 3, seed).astype(np.float64).reshape(H, W, 3)
    ph = hash_uniform(6, seed + 1).astype(np.float64)
    waves = np.stack([0.5 + 0.35 * np.sin(0.21 * x * (1 + c) + 0.13 * y + 6.28 * ph[c]) * np.cos(0.17 * y - 0.05 * x * c + 6.28 * ph[3 + c])
                      for c in range(3)], -1)
    return np.clip(0.6 * waves + 0.4 * u, 0.0, 1.0).astype(np.float32)


def make_pair(H, W, seed):
    """(img float32 [H,W,3], gt float64 [H,W,3]): an image, and the same image plus hash noise of amplitude NOISE (clipped to [0,1])"""
    gt = make_image(H, W, seed)
    n = (2.0 * hash_uniform(H * W * 3, seed + 5).astype(np.float64) - 1.0).reshape(H, W, 3) * NOISE
    img = np.clip(gt.astype(np.float64) + n, 0.0, 1.0).astype(np.float32)
    return img, gt.astype(np.float64)


def out_side(n, k, s, p, ceil=False):
    v = (n + 2 * p - k) / s
    return int(np.ceil(v) if ceil else np.floor(v)) + 1


def tap_shapes(net, H, W):
    """[(C, h, w)] of the five taps"""
    out, h, w = [None] * 5, H, W
    for op in ARCH[net]:
        if op[0] == "conv":
            h, w = out_side(h, op[3], op[4], op[5]), out_side(w, op[3], op[4], op[5])
            if op[6] is not None:
                out[op[6]] = (op[2], h, w)
        else:
            h, w = out_side(h, op[1], op[2], 0), out_side(w, op[1], op[2], 0)
    return out


def macs(net, H, W):
    """multiply-accumulates of the convolutions of ONE image (exact)"""
    total, h, w = 0, H, W
    for op in ARCH[net]:
        if op[0] == "conv":
            h, w = out_side(h, op[3], op[4], op[5]), out_side(w, op[3], op[4], op[5])
            total += h * w * op[2] * op[1] * op[3] * op[3]
        else:
            h, w = out_side(h, op[1], op[2], 0), out_side(w, op[1], op[2], 0)
    return total


def scaling_layer(stack, rgb_pm1=False, variant=None):
    """[n,H,W,3] (numpy / tensor; float64 inputs are cast to float32 first) -> [n,3,H,W] float32 tensor behind the scaling layer"""
    v = torch.as_tensor(np.asarray(stack)).to(torch.float32)
    x = v.permute(0, 3, 1, 2)
    if not rgb_pm1:
        x = 2.0 * x - 1.0
        if variant != "no_flip":
            x = x.flip(1)
    shift = torch.tensor(SHIFT, dtype=torch.float32).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=torch.float32).view(1, 3, 1, 1)
    return (x - shift) / scale


def features(net, weights, stack, dtype=torch.float64, rgb_pm1=False, variant=None):
    """the five taps [n,C,h,w] (tensors of `dtype`) of a stack [n,H,W,3]"""
    x = scaling_layer(stack, rgb_pm1, variant).to(dtype)
    taps, ci = [None] * 5, 0
    for op in ARCH[net]:
        if op[0] == "conv":
            _, _, _, k, s, p, tap = op
            if variant == "alex_stride3" and k == 11:
                s = 3
            w = torch.as_tensor(weights["conv"][ci][0]).to(dtype)
            b = torch.as_tensor(weights["conv"][ci][1]).to(dtype)
            ci += 1
            if variant == "replicate_pad":
                z = TF.conv2d(TF.pad(x, (p, p, p, p), mode="replicate"), w, b, stride=s)
            else:
                z = TF.conv2d(x, w, b, stride=s, padding=p)
            x = torch.relu(z)
            if tap is not None:
                taps[tap] = z if variant == "pre_relu_taps" else x
        else:
            x = TF.max_pool2d(x, op[1], op[2], ceil_mode=(variant == "ceil_pool"))
    return taps


def head(taps0, taps1, lins, variant=None):
    """(out [F], layers [F,5]) in the taps' dtype"""
    layers = []
    for f0, f1, w in zip(taps0, taps1, lins):
        w = torch.as_tensor(w).to(f0.dtype).view(1, -1, 1, 1)
        if variant == "eps_inside":
            n0 = f0 / torch.sqrt((f0 * f0).sum(1, keepdim=True) + 1e-10)
            n1 = f1 / torch.sqrt((f1 * f1).sum(1, keepdim=True) + 1e-10)
        else:
            n0 = f0 / (torch.sqrt((f0 * f0).sum(1, keepdim=True)) + 1e-10)
            n1 = f1 / (torch.sqrt((f1 * f1).sum(1, keepdim=True)) + 1e-10)
        layers.append((w * (n0 - n1) ** 2).sum(1).mean((1, 2)))
    layers = torch.stack(layers, 1)
    return layers.sum(1), layers


def lpips(net, weights, img, gt, dtype=torch.float64, rgb_pm1=False, variant=None):
    """img, gt [F,H,W,3] -> (out [F], layers [F,5]) numpy float64"""
    t0 = features(net, weights, img, dtype, rgb_pm1, variant)
    t1 = features(net, weights, gt, dtype, rgb_pm1, variant)
    out, layers = head(t0, t1, weights["lin"], variant)
    return out.double().numpy(), layers.double().numpy()


def border_mask(h, w):
    """[h,w] bool: the outermost ring of a tap (where the padding rule shows)"""
    m = np.zeros((h, w), bool)
    m[0, :] = m[-1, :] = True
    m[:, 0] = m[:, -1] = True
    return m
