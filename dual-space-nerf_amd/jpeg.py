"""Baseline JPEG on the device: the scripts' `cv2.imwrite(path, color_img.numpy() * 255)` into a .jpg (validate.py:76-83,
novel_pose_vis.py:62-66, vis_lighting.py:62-65, test.py) and img2vid's place, from frames that are in HBM already.

    encode(images, quality=95, subsampling="420", channels="bgr", scale=255.0) -> list[bytes]      two device->host copies per call
    encode_device(images, ...) -> (buffer uint8 [F, capacity], lengths int32 [F], status int32 [F])  on the device, no wait
    imwrite(path, img, params=None)                                                                   cv2.imwrite's shape, .jpg / .jpeg
    write_avi(path, files, fps)                                                                       Motion-JPEG AVI around encoded frames (host)
    decode(files, channels="bgr", gray=False) -> uint8 [H, W, 3] / [F, H, W, 3] on the device        the datasets' cv2.imread of a .jpg
    decode_device(files, ...) -> (pixels, status int32 [F], rounds int32 [F])                         one status copy per group of rounds
    imread(path) / imread_batch(paths)                                                                cv2.imread's shape: B, G, R

Decoding takes baseline files (SOF0, 8 bits, one interleaved scan, grey / 4:4:4 / 4:2:0, any 8-bit DQT and any DHT): the pixels are
the ones Pillow decodes through libjpeg-turbo at its default settings; cv2.imread's own pixels are not claimed.  The file bytes go up,
the frame appears in HBM; anything else (progressive, 4:2:2, restart intervals, ...) raises ValueError with the parser's reason.

The arithmetic is the rule written out in include/dsnerf.h and restated in tests/jpeg_restate.py: byte for byte the file Pillow
writes through libjpeg-turbo at the same quality and subsampling (optimize=False).  cv2.imwrite's own bytes are not claimed, and the
float -> level rule (v * scale, nearest-even, saturated, NaN -> 0) is what convertTo(CV_8U) is understood to do, unverified.

An image is [H, W, 3], [H, W, 1] or [H, W]; a stack has a leading F; a list holds equal-sized images.  uint8 or float32 (float64 is
cast to float32 first); host arrays are uploaded once.  One channel writes a one-component file whatever `subsampling` says.
"""
from __future__ import annotations

import os
import struct

import numpy as np
import torch

from . import _lib

NONFINITE, OVERFLOW = _lib.JPEG_NONFINITE, _lib.JPEG_OVERFLOW
IMWRITE_JPEG_QUALITY = 1          # cv2's constant


def _stack(images, device=None, what="jpeg"):
    """-> (contiguous device stack [F, H, W, 3] or [F, H, W], uint8 or float32)"""
    if isinstance(images, (list, tuple)):
        items = [torch.as_tensor(np.ascontiguousarray(x)) if not torch.is_tensor(x) else x for x in images]
        if not items:
            raise ValueError(f"{what}: an empty list of images")
        if any(x.shape != items[0].shape or x.dtype != items[0].dtype for x in items):
            raise ValueError(f"{what}: the images of a list must have one size and dtype (encode each size group on its own)")
        if items[0].dim() not in (2, 3):
            raise ValueError(f"{what}: a list holds images [H, W], [H, W, 1] or [H, W, 3], got {tuple(items[0].shape)}")
        x = torch.stack(items)
    else:
        x = images if torch.is_tensor(images) else torch.as_tensor(np.ascontiguousarray(images))
        if x.dim() == 2 or (x.dim() == 3 and x.shape[2] in (1, 3)):
            x = x.unsqueeze(0)
    if x.dim() == 4 and x.shape[3] == 1:
        x = x[..., 0]
    if x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[3] != 3):
        raise ValueError(f"{what}: images must be [H, W], [H, W, 1], [H, W, 3] or a stack of them, got {tuple(x.shape)}")
    if x.dtype == torch.float64:
        x = x.to(torch.float32)
    if x.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"{what}: images must be uint8 or float32 (float64 is cast), got {x.dtype}")
    if not x.is_cuda:
        _lib.require_gpu()
        x = x.to(torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device()))
    return x.contiguous()


def _args(quality, channels):
    if int(quality) != quality or not 1 <= int(quality) <= 100:
        raise ValueError(f"jpeg: quality must be an integer 1 ... 100, got {quality!r}")
    if channels not in ("bgr", "rgb"):
        raise ValueError(f"jpeg: channels must be 'bgr' or 'rgb', got {channels!r}")
    return int(quality), channels == "rgb"


def encode_device(images, quality=95, subsampling="420", channels="bgr", scale=255.0, capacity=None, device=None):
    """-> (buffer uint8 [F, capacity]: row f starts with frame f's complete file, lengths int32 [F], status int32 [F]: OR of
    NONFINITE / OVERFLOW) on the device; nothing is copied back and nothing waits.  capacity: bytes per row, by default
    dsn_jpeg_max_bytes (no frame can overflow it)."""
    q, rgb = _args(quality, channels)
    x = _stack(images, device)
    mode = _lib.jpeg_mode(subsampling, 3 if x.dim() == 4 else 1)
    return _lib.jpeg_encode(x, mode, q, rgb, scale, capacity=capacity)


def encode(images, quality=95, subsampling="420", channels="bgr", scale=255.0, device=None):
    """-> one `bytes` per frame.  Two device->host copies whatever F is: the lengths (with the status words), then the used bytes."""
    buf, lengths, status = encode_device(images, quality, subsampling, channels, scale, device=device)
    head = torch.stack([lengths, status]).cpu().numpy()          # copy 1
    n = [int(v) for v in head[0]]
    if any(int(s) & OVERFLOW for s in head[1]):                  # (cannot happen at the default capacity)
        raise RuntimeError("jpeg.encode: a frame did not fit dsn_jpeg_max_bytes")
    used = buf[:, :max(n)].cpu().numpy()                         # copy 2
    return [used[f, :n[f]].tobytes() for f in range(len(n))]


def _quality_of(params):
    q = 95
    if params:
        p = [int(v) for v in params]
        if len(p) % 2:
            raise ValueError(f"imwrite: params must be (flag, value) pairs, got {params!r}")
        for flag, value in zip(p[0::2], p[1::2]):
            if flag != IMWRITE_JPEG_QUALITY:
                raise ValueError(f"imwrite: the only flag taken is IMWRITE_JPEG_QUALITY (1), got {flag}")
            q = value
    return q


def imwrite(path, img, params=None):
    """cv2.imwrite(path, img, params)'s shape for .jpg / .jpeg: img [H, W, 3] in B, G, R order (or [H, W], [H, W, 1]); uint8 levels, or
    float levels that are rounded and saturated as convertTo(CV_8U) does (the scripts pass `color_img * 255`): scale = 1 here.
    params: [IMWRITE_JPEG_QUALITY, q].  Returns True."""
    if os.path.splitext(str(path))[1].lower() not in (".jpg", ".jpeg"):
        hint = " - dsnerf_amd.png.imwrite writes those" if os.path.splitext(str(path))[1].lower() == ".png" else ""
        raise ValueError(f"imwrite: only .jpg / .jpeg files are written, got {path!r}{hint}")
    data = encode(img, quality=_quality_of(params), scale=1.0)
    if len(data) != 1:
        raise ValueError("imwrite: one image per file")
    with open(path, "wb") as f:
        f.write(data[0])
    return True


def _jpeg_size(data):
    """(W, H) from the SOF0 segment"""
    i = 2
    while i + 4 <= len(data) and data[i] == 0xFF:
        n = int.from_bytes(data[i + 2:i + 4], "big")
        if data[i + 1] == 0xC0:
            return int.from_bytes(data[i + 7:i + 9], "big"), int.from_bytes(data[i + 5:i + 7], "big")
        i += 2 + n
    raise ValueError("write_avi: no SOF0 segment: not a baseline JPEG")


def _chunk(tag, payload):
    return tag + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def write_avi(path, files, fps=30):
    """A Motion-JPEG AVI around already encoded frames (img2vid's place; host code): `files` are paths of .jpg files or `bytes`
    objects, all of one size.  RIFF 'AVI ': LIST hdrl (avih, LIST strl (strh vids/MJPG, strf BITMAPINFOHEADER)), LIST movi of
    '00dc' chunks, idx1 with offsets relative to the 'movi' tag.  Returns the number of frames."""
    frames = []
    for f in files:
        if isinstance(f, (bytes, bytearray, memoryview)):
            frames.append(bytes(f))
        else:
            with open(f, "rb") as h:
                frames.append(h.read())
    if not frames:
        raise ValueError("write_avi: no frames")
    if not fps > 0:
        raise ValueError(f"write_avi: fps must be positive, got {fps!r}")
    W, H = _jpeg_size(frames[0])
    for k, d in enumerate(frames):
        if d[:2] != b"\xff\xd8" or _jpeg_size(d) != (W, H):
            raise ValueError(f"write_avi: frame {k} is not a JPEG of {W} x {H}")
    n, biggest = len(frames), max(len(d) for d in frames)
    rate, scale = (int(fps), 1) if float(fps) == int(fps) else (int(round(fps * 1000)), 1000)
    avih = struct.pack("<14I", int(round(1e6 * scale / rate)), int(biggest * rate / scale), 0, 0x10, n, 0, 1, biggest, W, H, 0, 0, 0, 0)
    strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIIIhhhh", 0, 0, 0, 0, scale, rate, 0, n, biggest, 0xFFFFFFFF, 0, 0, 0, W, H)
    strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0)
    hdrl = b"hdrl" + _chunk(b"avih", avih) + _chunk(b"LIST", b"strl" + _chunk(b"strh", strh) + _chunk(b"strf", strf))
    movi, idx, off = b"movi", b"", 4
    for d in frames:
        c = _chunk(b"00dc", d)
        idx += b"00dc" + struct.pack("<III", 0x10, off, len(d))
        movi += c
        off += len(c)
    body = b"AVI " + _chunk(b"LIST", hdrl) + _chunk(b"LIST", movi) + _chunk(b"idx1", idx)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    return n


# ---- decoding ---------------------------------------------------------------------------------------------------------------------------------
def _parse_all(files, names):
    descs = []
    for k, f in enumerate(files):
        d, st = _lib.jpeg_parse(f)
        if st != 0:
            hint = " - a PNG file: dsnerf_amd.png.imread / png.decode read those" if f[:8] == b"\x89PNG\r\n\x1a\n" else ""
            raise ValueError(f"jpeg.decode: {names[k]}: not a file this decoder takes ({_lib.JPEGD_REASONS[st]}){hint}")
        descs.append(d)
    return descs


def _groups(descs):
    """indices grouped by (H, W, mode), in order of first appearance (as save_views groups on the way out)"""
    g = {}
    for k, d in enumerate(descs):
        g.setdefault((int(d.H), int(d.W), int(d.mode)), []).append(k)
    return list(g.values())


def _decode_groups(files, names, channels, gray, device, subseq_bits):
    if channels not in ("bgr", "rgb"):
        raise ValueError(f"jpeg: channels must be 'bgr' or 'rgb', got {channels!r}")
    files = [bytes(f) for f in files]
    if not files:
        raise ValueError("jpeg.decode: an empty list of files")
    descs = _parse_all(files, names)
    out, status, rounds = [None] * len(files), [0] * len(files), [0] * len(files)
    for idx in _groups(descs):
        batch = _lib.JpegdBatch([files[k] for k in idx], [descs[k] for k in idx], device)
        px, st, rd, host = _lib.jpeg_decode(batch, subseq_bits, rgb=channels == "rgb", gray=gray)
        for j, k in enumerate(idx):
            out[k], status[k], rounds[k] = px[j], int(host[0, j]), int(host[1, j])
    return out, status, rounds


def _names(files, names):
    return list(names) if names is not None else [f"file {k}" for k in range(len(files))]


def decode_device(files, channels="bgr", gray=False, device=None, subseq_bits=None, names=None):
    """files: one `bytes` or a list of them -> (pixels, status, rounds).  pixels: a uint8 device tensor [F, H, W, 3] (gray: [F, H, W])
    when all files share a size and sampling mode, else a list of [H, W, 3] tensors in the files' order; status / rounds: int32 [F]
    host arrays (DSN_JPEGD_* bits; the synchronisation rounds each frame took).  A corrupt frame is all zeros and keeps its bit set:
    nothing is raised here."""
    single = isinstance(files, (bytes, bytearray, memoryview))
    files = [files] if single else list(files)
    out, status, rounds = _decode_groups(files, _names(files, names), channels, gray, device, subseq_bits)
    same = all(o.shape == out[0].shape for o in out)
    px = torch.stack(out) if same else out
    return px, np.asarray(status, np.int32), np.asarray(rounds, np.int32)


def decode(files, channels="bgr", gray=False, device=None, subseq_bits=None, names=None):
    """One `bytes` -> a uint8 device tensor [H, W, 3] in B, G, R order (what cv2.imread returns; channels="rgb": R, G, B; gray=True, for
    one-component files: [H, W]).  A list -> [F, H, W, 3] when sizes and modes agree, else a list of tensors.  An unsupported or corrupt
    file raises ValueError naming the file and the reason."""
    single = isinstance(files, (bytes, bytearray, memoryview))
    lst = [files] if single else list(files)
    nm = _names(lst, names)
    px, status, _ = decode_device(lst, channels, gray, device, subseq_bits, nm)
    for k, st in enumerate(status):
        if int(st) & _lib.JPEGD_CORRUPT:
            why = [n for n, b in (("a code that matches nothing", _lib.JPEGD_UNMATCHED), ("a coefficient index past 63", _lib.JPEGD_OVERRUN),
                                  ("a marker inside the scan", _lib.JPEGD_MARKER), ("a block count that is not the frame's", _lib.JPEGD_COUNT))
                   if int(st) & b]
            raise ValueError(f"jpeg.decode: {nm[k]}: corrupt scan ({', '.join(why)})")
    return px[0] if single else px


def imread_batch(paths, channels="bgr", device=None):
    """the files at `paths` -> as decode() of their bytes"""
    data = []
    for p in paths:
        if str(p).lower().endswith(".png"):
            raise ValueError(f"jpeg.imread: {p}: a .png path - dsnerf_amd.png.imread reads those")
        with open(p, "rb") as f:
            data.append(f.read())
    return decode(data, channels=channels, device=device, names=[str(p) for p in paths])


def imread(path, channels="bgr", device=None):
    """cv2.imread(path)'s shape for a .jpg: uint8 [H, W, 3] in B, G, R order, on the device"""
    return imread_batch([path], channels, device)[0]
