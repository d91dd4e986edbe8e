"""Writes tests/golden/jpeg_decode_pillow.npz: small JPEG files written by Pillow (libjpeg-turbo) and the pixels Pillow decodes from
them, for tests/test_jpeg_decode_host.py and tests/test_gpu_jpeg_decode.py where Pillow itself may not import.

    python tests/golden/make_golden_jpeg_decode.py

meta: lines "key H W sub quality kind"; jpg_<key>: the file; px_<key>: Pillow's pixels ([H, W, 3] R, G, B or [H, W]).
ext_jpg_<q> / ext_px_<q>: files around the 128 extreme blocks' coefficients (jpeg_restate.scan_file) under the tables of quality q,
decoded by Pillow: at its default settings for q = 100 and 99; for q = 98, 95 and 75, where samples leave [-512, 511] before the range
limit, in a child process with JSIMD_FORCENONE=1, which makes libjpeg-turbo run jidctint.c itself (its 16-bit SIMD IDCT saturates
where jidctint.c wraps; no 8-bit encoder writes such coefficients).
refused: lines "name reason"; refused_<name>: a file the parser refuses for that reason.
rounds_<B>: the synchronisation rounds of every meta file at B bits per subsequence (jpeg_decode_restate.coefficients)."""
import io
import os
import subprocess
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_decode_restate as JD  # noqa: E402
import jpeg_restate as JR  # noqa: E402

SIZES = [(1, 1), (2, 3), (3, 2), (5, 4), (4, 5), (1, 6), (6, 1), (9, 5), (16, 16), (17, 33), (37, 53), (130, 70)]
SUBS = {"420": 2, "444": 0}


def image(rng, H, W, kind):
    y, x = np.mgrid[0:H, 0:W]
    smooth = np.stack([(128 + 100 * np.sin(x / 9.0 + k) * np.cos(y / 7.0 + 0.3 * k)) for k in range(3)], -1)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return np.clip(smooth + rng.integers(-6, 7, (H, W, 3)), 0, 255).astype(np.uint8)


def save(img, sub, **kw):
    b = io.BytesIO()
    if sub != "gray":
        kw["subsampling"] = SUBS[sub]
    Image.fromarray(img).save(b, "JPEG", **kw)
    return b.getvalue()


def pillow_pixels(data):
    return np.asarray(Image.open(io.BytesIO(data)))


def pillow_pixels_scalar(data):
    """Pillow's pixels with libjpeg-turbo's SIMD off (jidctint.c's jpeg_idct_islow itself): the variable is read once per process"""
    code = "import sys, io, numpy as np; from PIL import Image; b = io.BytesIO(); np.save(b, np.asarray(Image.open(io.BytesIO(sys.stdin.buffer.read())))); sys.stdout.buffer.write(b.getvalue())"
    r = subprocess.run([sys.executable, "-c", code], input=data, stdout=subprocess.PIPE, check=True, env={**os.environ, "JSIMD_FORCENONE": "1"})
    return np.load(io.BytesIO(r.stdout))


def extreme_coefficients():
    """the quantised (quality 100: all entries 1) coefficients of the encoder tests' 128 extreme blocks, one row of grey 8 x 8 MCUs"""
    k = np.arange(8)
    A = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * np.where(k == 0, np.sqrt(1 / 8), 0.5)[:, None]
    ext = np.stack([np.where(np.outer(A[u], A[v]) >= 0, 127, -128) for u in range(8) for v in range(8)])
    blocks = np.concatenate([ext, -ext - 1])
    z = JR.quantise(JR.fdct(blocks), JR.quant_tables(100)[0]).reshape(-1, 64)[:, JR.ZIGZAG]
    return z.astype(np.int16)


def refused_files(rng):
    img = image(rng, 16, 16, "smooth")
    good = save(img, "420", quality=90)
    head, scan, tail = JR.split_file(good)
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=90, subsampling=1)
    out = {"progressive": (save(img, "420", quality=90, progressive=True), "progressive"), "s422": (b.getvalue(), "sampling"),
           "restart": (save(img, "420", quality=90, restart_marker_blocks=1), "restart")}
    i = good.index(b"\xff\xdb")
    out["table16"] = (good[:i + 4] + bytes([0x10]) + good[i + 5:], "table16")
    s = good.index(b"\xff\xda")
    out["two_scans"] = (good[:s] + bytes([0xFF, 0xDA, 0, 8, 1, 1, 0x00, 0, 63, 0]) + scan + tail, "multiscan")
    out["truncated_header"] = (good[:300], "truncated")
    f = good.index(b"\xff\xc0")
    out["twelve_bits"] = (good[:f + 4] + bytes([12]) + good[f + 5:], "precision")
    out["arithmetic"] = (good[:f + 1] + bytes([0xC9]) + good[f + 2:], "arithmetic")
    out["no_eoi"] = (good[:-2], "no_eoi")
    out["not_jpeg"] = (b"\x89PNG\r\n\x1a\n" + good[8:], "not_jpeg")
    return out


def main():
    rng = np.random.default_rng(2026)
    out, meta = {}, []

    def add(key, H, W, sub, q, kind, data):
        meta.append(f"{key} {H} {W} {sub} {q} {kind}")
        out[f"jpg_{key}"] = np.frombuffer(data, np.uint8)
        out[f"px_{key}"] = pillow_pixels(data)

    n = 0
    for H, W in SIZES:
        for sub in ("420", "444", "gray"):
            for q in (1, 50, 95, 100):
                if H * W > 37 * 53 and q in (1, 100):
                    continue
                kind = "noise" if q in (95, 100) else "smooth"
                img = image(rng, H, W, kind)
                img = img[..., 0] if sub == "gray" else img
                add(f"c{n}", H, W, sub, q, kind, save(img, sub, quality=q))
                n += 1
    for H, W in ((17, 33), (37, 53), (5, 4)):
        for sub in ("420", "444", "gray"):
            img = image(rng, H, W, "smooth")
            img = img[..., 0] if sub == "gray" else img
            add(f"o{n}", H, W, sub, 75, "optimize", save(img, sub, quality=75, optimize=True))
            n += 1
            qt = [[int(v) for v in rng.integers(1, 64, 64)], [int(v) for v in rng.integers(1, 256, 64)]]
            add(f"q{n}", H, W, sub, 0, "qtables", save(img, sub, qtables=qt[:1] if sub == "gray" else qt))
            n += 1
    img = image(rng, 37, 53, "smooth")
    data = save(img, "420", quality=85, comment=b"a comment segment", exif=b"Exif\0\0MM\0*\0\0\0\x08\0\0\0\0\0\0")
    assert b"\xff\xfe" in data and b"\xff\xe1" in data
    add(f"s{n}", 37, 53, "420", 85, "segments", data)
    coef = extreme_coefficients()
    for q in (100, 99, 98, 95, 75):
        data = JR.scan_file(coef, 8, 8 * len(coef), JR.MGRAY, q)
        out[f"ext_jpg_{q}"] = np.frombuffer(data, np.uint8)
        out[f"ext_px_{q}"] = pillow_pixels(data) if q >= 99 else pillow_pixels_scalar(data)
    refused = refused_files(rng)
    out["refused"] = np.array([f"{k} {v[1]}" for k, v in refused.items()])
    for k, v in refused.items():
        out[f"refused_{k}"] = np.frombuffer(v[0], np.uint8)
    out["meta"] = np.array(meta)
    for B in (128, 160, 1024):
        out[f"rounds_{B}"] = np.array([JD.coefficients(out[f"jpg_{m.split()[0]}"].tobytes(), B)[2] for m in meta], np.int32)
    path = os.path.join(HERE, "jpeg_decode_pillow.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(meta), "files")


if __name__ == "__main__":
    main()
