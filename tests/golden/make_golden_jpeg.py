"""Writes tests/golden/jpeg_pillow.npz: small images with the bytes Pillow (libjpeg-turbo) wrote for them, optimize=False.

    python tests/golden/make_golden_jpeg.py

Keys: img_<k> uint8 [H, W, 3] (R, G, B) or [H, W]; jpg_<k> uint8 bytes; meta: one line per case "k H W subsampling quality content"."""
import io
import os

import numpy as np
from PIL import Image

SIZES = [(1, 1), (7, 5), (8, 8), (16, 17), (17, 9), (37, 53), (40, 48), (63, 65)]
QUALITIES = [10, 50, 95, 100]
SUBS = ["420", "444", "gray"]


def content(kind, H, W, C, rng):
    if kind == "noise":
        return rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([(128 + 100 * np.sin(x / 9.0 + k) * np.cos(y / 7.0 + 0.3 * k)).astype(np.uint8) for k in range(C)], -1)


def main():
    rng = np.random.default_rng(2026)
    out, meta = {}, []
    k = 0
    for i, (H, W) in enumerate(SIZES):
        for j, sub in enumerate(SUBS):          # every size in every mode; qualities and contents rotate
            q = QUALITIES[(i + j) % 4]
            kind = "noise" if (i + j) % 2 == 0 else "smooth"
            C = 1 if sub == "gray" else 3
            img = content(kind, H, W, C, rng)
            b = io.BytesIO()
            if C == 1:
                Image.fromarray(img[..., 0]).save(b, "JPEG", quality=q, optimize=False)
                img = img[..., 0]
            else:
                Image.fromarray(img).save(b, "JPEG", quality=q, subsampling={"444": 0, "420": 2}[sub], optimize=False)
            out[f"img_{k}"] = img
            out[f"jpg_{k}"] = np.frombuffer(b.getvalue(), np.uint8)
            meta.append(f"{k} {H} {W} {sub} {q} {kind}")
            k += 1
    out["meta"] = np.array(meta)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_pillow.npz")
    np.savez_compressed(path, **out)
    print(path, k, "cases", os.path.getsize(path), "bytes; Pillow", Image.__version__)


if __name__ == "__main__":
    main()
