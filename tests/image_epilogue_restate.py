"""numpy statements of the image epilogue (csrc/dsn_image.hip) for tests/test_gpu_image_epilogue.py and test_image_epilogue_host.py.

scatter            post_process by numpy boolean-mask assignment: the rule itself (rows of the compacted arrays go, in order, to the set
                   pixels; a set pixel whose rank is R or more, and every other pixel, is zero)
scatter_by_scan    the same image the way the kernels reach it - per-block counts, the single-workgroup exclusive scan in trips of 1024
                   blocks with a carry, rank = block offset + prefix inside the block; carry=False is the mutant that drops the carry
squared_errors     per-pixel float64 squared error as k_img_sqerr forms it: (double)img - gt, three squares added in channel order
psnr_reference     the four numbers of dsn_image_psnr from math.fsum (exact sums, rounded once); divide_by_n=True is the mutant that
                   divides the masked sum by the pixel count
psnr_bars          the derived bars on those numbers
psnr_errors        the errors the bars apply to; a NaN where a finite value is expected is an assertion error, never a small error
"""
import math

import numpy as np

BLOCK = 256           # IMG_THREADS
TRIP = 1024           # blocks per trip of k_img_scan
MAX_BLOCKS = 1024     # the launch cap of k_img_sqerr


SCATTER_SIZES = [(512, 512), (513, 512), (1024, 513)]          # 1024 blocks (one scan trip), 1026 (the first carry), 2052 (two carries)


def scatter_masks(H, W):
    """name -> [H * W] bool: the masks of the scatter tests"""
    n = H * W
    rng = np.random.default_rng(H * 1000 + W)
    out = {"random": rng.random(n) < 0.5, "empty": np.zeros(n, bool), "full": np.ones(n, bool)}
    for name, pixels in (("first of block 1024", [262144]), ("last", [n - 1])):
        if pixels[0] < n:
            out[name] = np.zeros(n, bool)
            out[name][pixels] = True
    out["blocks 1023-1025"] = np.zeros(n, bool)
    out["blocks 1023-1025"][1023 * 256:1026 * 256] = True
    return out


def scatter(src, mask, R, clamp=False):
    """src [rows, c] float32 (rows >= R), mask [n] bool -> [n, c] float32"""
    mask = np.asarray(mask, bool).reshape(-1)
    src = np.asarray(src, np.float32).reshape(len(src), -1)
    rows = np.zeros((int(mask.sum()), src.shape[1]), np.float32)
    k = min(R, len(rows))
    rows[:k] = np.clip(src[:k], 0.0, 1.0) if clamp else src[:k]          # np.clip keeps NaN, as torch.clamp does
    out = np.zeros((mask.size, src.shape[1]), np.float32)
    out[mask] = rows
    return out


def block_offsets(mask, carry=True):
    """exclusive scan of the per-block popcounts, as k_img_scan walks it"""
    n = mask.size
    nblocks = -(-n // BLOCK)
    padded = np.zeros(nblocks * BLOCK, np.int64)
    padded[:n] = mask
    counts = padded.reshape(nblocks, BLOCK).sum(1)
    offs = np.zeros(nblocks, np.int64)
    c = 0
    for base in range(0, nblocks, TRIP):
        v = counts[base:base + TRIP]
        inc = np.cumsum(v)
        offs[base:base + TRIP] = c + inc - v
        if carry:
            c += int(inc[-1])
    return offs


def scatter_by_scan(src, mask, R, clamp=False, carry=True):
    mask = np.asarray(mask, bool).reshape(-1)
    src = np.asarray(src, np.float32).reshape(len(src), -1)
    n = mask.size
    offs = block_offsets(mask, carry)
    nblocks = len(offs)
    padded = np.zeros(nblocks * BLOCK, np.int64)
    padded[:n] = mask
    inside = np.cumsum(padded.reshape(nblocks, BLOCK), 1) - padded.reshape(nblocks, BLOCK)
    rank = (offs[:, None] + inside).reshape(-1)[:n]
    take = mask & (rank < R)
    out = np.zeros((n, src.shape[1]), np.float32)
    v = src[rank[take]]
    out[take] = np.clip(v, 0.0, 1.0) if clamp else v
    return out


def squared_errors(img, gt):
    """[n] float64; img float32 [n,3], gt float64 or float32 [n,3]"""
    img, gt = np.asarray(img).reshape(-1, 3), np.asarray(gt).reshape(-1, 3)
    assert img.dtype == np.float32 and gt.dtype in (np.float64, np.float32)
    d = img.astype(np.float64) - gt.astype(np.float64)
    sq = d * d
    return (sq[:, 0] + sq[:, 1]) + sq[:, 2]


def _exact(e):
    return float("nan") if np.isnan(e).any() else math.fsum(e.tolist())


def psnr_reference(e, mask=None, divide_by_n=False):
    """{mse_all, mse_masked, psnr_all, psnr_masked} as float64 from the per-pixel errors e [n]; no mask: the masked two are 0 / 0"""
    n = e.size
    with np.errstate(divide="ignore", invalid="ignore"):
        mse_all = np.float64(_exact(e)) / np.float64(3.0 * n)
        if mask is None:
            s, count = 0.0, 0
        else:
            m = np.asarray(mask, bool).reshape(-1)
            s, count = _exact(e[m]), int(m.sum())
        mse_m = np.float64(s) / np.float64(3.0 * (n if divide_by_n else count))
        return np.array([mse_all, mse_m, -10.0 * np.log10(mse_all), -10.0 * np.log10(mse_m)])


def additions(n):
    """D: the most additions a term of the sum passes through - the thread's grid-stride loop (ceil(n / (256 B)) terms), the 8 levels
    of the block's tree, and B atomic additions in any order; B = min(1024, blocks)"""
    B = min(MAX_BLOCKS, -(-n // BLOCK))
    return -(-n // (BLOCK * B)) + 8 + B


def psnr_bars(n):
    """(relative bar on mse, absolute bar on psnr): all terms are non-negative, so |sum - exact| <= D 2^-53 exact; the division
    keeps the relative error and -10 log10 turns it into 10 D 2^-53 / ln 10.
    Left out on purpose: the roundings of the division, of log10 and of the multiplication by 10 - on the device and in the
    reference alike, up to two or three ulps of the value between them (an ulp of a 10 ... 30 dB psnr is 1.8e-15 ... 3.6e-15).  D >= 10
    covers them from 512 x 512 on a hundred times over; at the smallest sizes (D = 10: bars 1.1e-15 and 4.8e-15) the bar is about
    one ulp of 30 dB, so a device log10 one ulp off numpy's could miss it there without any summation error.  The bar is kept as
    derived from the sum alone: such a miss would be a finding about log10, to be read as one."""
    D = additions(n)
    return D * 2.0 ** -53, 10.0 * D * 2.0 ** -53 / math.log(10.0)


def psnr_errors(got, want):
    """(largest relative error of the two mse, largest absolute error of the two psnr) of the four numbers `got` against `want`.
    Where `want` is NaN, infinite or zero, `got` must be that very value (it then counts as error 0); where `want` is finite,
    `got` must be finite too - a NaN in its place raises, it never compares as a small error."""
    got, want = np.asarray(got, np.float64).reshape(4), np.asarray(want, np.float64).reshape(4)
    out = []
    for idx in ((0, 1), (2, 3)):
        worst = 0.0
        for i in idx:
            if not np.isfinite(want[i]) or want[i] == 0:
                assert np.array_equal(got[i], want[i], equal_nan=True), (i, got.tolist(), want.tolist())
            else:
                assert np.isfinite(got[i]), (i, got.tolist(), want.tolist())
                err = abs(got[i] - want[i]) / (abs(want[i]) if i < 2 else 1.0)
                worst = err if not err <= worst else worst
        out.append(float(worst))
    return out
