"""PNG on the device.

Encoding: test.py's five `cv2.imwrite(....png)` per evaluated frame (test.py:94-110), from frames that are in HBM already:
    encode(images, channels="bgr", scale=255.0, replicate=False, filter="adaptive", chunk=None) -> list[bytes]   two device->host copies per call
    encode_device(images, ...) -> (buffer uint8 [F, capacity], lengths int32 [F], status int32 [F])              on the device, no wait
    imwrite(path, img, params=None)                                                                               cv2.imwrite's shape, .png
An image is [H, W, 3], [H, W, 1] or [H, W]; a stack has a leading F; a list holds equal-sized images.  uint8 or float32 (float64 is
cast to float32 first); host arrays are uploaded once.  Three channels give an 8-bit RGB file, one channel an 8-bit grey one or, with
replicate=True, an RGB file of three equal channels (test.py's np.repeat(..., 3, axis=2)) that never exist in memory.  The float ->
level rule is the JPEG writer's (v * scale, nearest-even, saturated, NaN -> 0: what convertTo(CV_8U) is understood to do, unverified);
cv2.imwrite's own bytes are not claimed.  The file is the one the rule in include/dsnerf.h gives (tests/png_encode_restate.py): adaptive
filters by libpng's heuristic, deflate in independent chunks with matches at distances 1, one pixel and one row, one dynamic Huffman
code per chunk.  Not written: 16-bit, alpha, palette and Adam7 files.

Decoding: the datasets' label masks (mask_cihp/....png - cv2.imread at dataloader/zju_mocap_dataset.py:197 and
zju_novel_pose_dataset.py:195, imageio.imread at h36m_dataset.py:81, h36m_dataset_test.py:81, novel_poses_dataset.py:70).  File bytes
go up, the uint8 mask that imageprep.prepare_zju / prepare_h36m take appears in HBM:
    decode(files, channels="bgr", first_channel=False) -> uint8 [H, W, 3] / [F, H, W, 3] on the device; ValueError for a corrupt stream
    decode_device(files, ...) -> (pixels, status int32 [F]), both on the device: nothing raised, a corrupt frame is zeros with its bits
    imread(path) / imread_batch(paths)                                                                cv2.imread's shape: B, G, R

channels: "bgr" is what cv2.imread(path) is understood to return - always three channels: grey replicated, the palette looked up,
alpha dropped (UNVERIFIED against OpenCV, which is not installed where the tests run; imageio is not either); "rgb" the same in the
other order; "native" what Pillow's np.asarray(Image.open(path)) holds for modes L / RGB / RGBA / LA (a 1-bit file as 0 / 255) and the
palette INDEX plane for P.  first_channel=True gives [H, W]: the `[..., 0]` both data sets take, without three channels ever
existing.

Accepted: non-interlaced files of colour type 0 and 3 (1, 2, 4, 8 bits), 2, 4 and 6 (8 bits), any split into IDAT chunks, any zlib
stream (stored, fixed and dynamic blocks); ancillary chunks are skipped (tRNS and gAMA are not applied).  Everything else - Adam7,
16-bit samples, a CRC mismatch, a missing chunk, a zlib header that is not plain deflate - raises ValueError naming the file and the
reason before anything reaches the device.  The rule is written out in include/dsnerf.h and restated in tests/png_decode_restate.py;
PNG is lossless, so the pixels are the ones every decoder gives."""
import os

import torch

from . import _lib
from .jpeg import _stack

STATUS_NAMES = _lib.PNG_STATUS_NAMES
NONFINITE, OVERFLOW = _lib.PNGE_NONFINITE, _lib.PNGE_OVERFLOW
IMWRITE_PNG_COMPRESSION = 16          # cv2's constant


# ---- encoding -----------------------------------------------------------------------------------------------------------------------------------
def encode_device(images, channels="bgr", scale=255.0, replicate=False, filter="adaptive", chunk=None, stored_only=False, capacity=None,
                  device=None):
    """-> (buffer uint8 [F, capacity]: row f starts with frame f's complete file, lengths int32 [F], status int32 [F]: OR of
    NONFINITE / OVERFLOW) on the device; nothing is copied back and nothing waits.  capacity: bytes per row, by default
    dsn_png_encode_max_bytes (no frame can overflow it).  chunk: bytes of the raw stream per independent deflate chunk, a power of two
    from 256 to 32768 (None: the library's default).  stored_only: no compression at all."""
    if channels not in ("bgr", "rgb"):
        raise ValueError(f"png: channels must be 'bgr' or 'rgb', got {channels!r}")
    f = _lib.pnge_filter(filter)
    c = _lib.pnge_chunk(chunk)
    x = _stack(images, device, "png")
    return _lib.png_encode(x, _lib.pnge_mode(x, replicate), channels == "rgb", scale, f, c, stored_only, capacity=capacity)


def encode(images, channels="bgr", scale=255.0, replicate=False, filter="adaptive", chunk=None, stored_only=False, device=None):
    """-> one `bytes` per frame.  Two device->host copies whatever F is: the lengths (with the status words), then the used bytes."""
    buf, lengths, status = encode_device(images, channels, scale, replicate, filter, chunk, stored_only, device=device)
    head = torch.stack([lengths, status]).cpu().numpy()          # copy 1
    n = [int(v) for v in head[0]]
    if any(int(s) & OVERFLOW for s in head[1]):                  # (cannot happen at the default capacity)
        raise RuntimeError("png.encode: a frame did not fit dsn_png_encode_max_bytes")
    used = buf[:, :max(n)].cpu().numpy()                         # copy 2
    return [used[f, :n[f]].tobytes() for f in range(len(n))]


def _stored_only_of(params):
    stored = False
    if params:
        p = [int(v) for v in params]
        if len(p) % 2:
            raise ValueError(f"imwrite: params must be (flag, value) pairs, got {params!r}")
        for flag, value in zip(p[0::2], p[1::2]):
            if flag != IMWRITE_PNG_COMPRESSION:
                raise ValueError(f"imwrite: the only flag taken is IMWRITE_PNG_COMPRESSION (16), got {flag}")
            stored = value == 0
    return stored


def imwrite(path, img, params=None):
    """cv2.imwrite(path, img, params)'s shape for .png: img [H, W, 3] in B, G, R order (or [H, W], [H, W, 1]); uint8 levels, or float
    levels that are rounded and saturated as convertTo(CV_8U) does (test.py passes `img * 255`): scale = 1 here.
    params: [IMWRITE_PNG_COMPRESSION, 0] writes stored blocks only; any other value takes the normal path.  Returns True."""
    ext = os.path.splitext(str(path))[1].lower()
    if ext != ".png":
        hint = " - dsnerf_amd.jpeg.imwrite writes those" if ext in (".jpg", ".jpeg") else ""
        raise ValueError(f"imwrite: only .png files are written, got {path!r}{hint}")
    data = encode(img, scale=1.0, stored_only=_stored_only_of(params))
    if len(data) != 1:
        raise ValueError("imwrite: one image per file")
    with open(path, "wb") as f:
        f.write(data[0])
    return True


# ---- decoding -----------------------------------------------------------------------------------------------------------------------------------


def _names(files, names):
    return list(names) if names is not None else [f"file {k}" for k in range(len(files))]


def _parse_all(files, names):
    descs, segs = [], []
    for k, f in enumerate(files):
        d, s, st = _lib.png_parse(f)
        if st != 0:
            hint = " - a JPEG file: dsnerf_amd.jpeg.imread / jpeg.decode read those" if f[:2] == b"\xff\xd8" else ""
            raise ValueError(f"png.decode: {names[k]}: not a file this decoder takes ({_lib.PNG_REASONS[st]}){hint}")
        descs.append(d)
        segs.append(s)
    return descs, segs


def _groups(descs):
    """indices grouped by (W, H, bit depth, colour type), in order of first appearance"""
    g = {}
    for k, d in enumerate(descs):
        g.setdefault((int(d.W), int(d.H), int(d.bits), int(d.ctype)), []).append(k)
    return list(g.values())


def _decode_groups(files, names, channels, first_channel, device):
    if channels not in _lib.PNG_CHANNELS:
        raise ValueError(f"png: channels must be 'bgr', 'rgb' or 'native', got {channels!r}")
    files = [bytes(f) for f in files]
    if not files:
        raise ValueError("png.decode: an empty list of files")
    descs, segs = _parse_all(files, names)
    groups = _groups(descs)
    out, status = [None] * len(files), [None] * len(files)
    whole = None
    for idx in groups:
        batch = _lib.PngBatch([files[k] for k in idx], [descs[k] for k in idx], [segs[k] for k in idx], device)
        px, st = _lib.png_decode(batch, channels, first_channel)
        if len(groups) == 1:
            whole = (px, st)
        for j, k in enumerate(idx):
            out[k], status[k] = px[j], st[j]
    return out, status, whole


def decode_device(files, channels="bgr", first_channel=False, device=None, names=None):
    """files: one `bytes` or a list of them -> (pixels, status), both on the device, nothing copied back and nothing raised for a corrupt
    stream: such a frame is all zeros and keeps its DSN_PNG_* bits.  pixels: uint8 [F, H, W, C] ([F, H, W] with first_channel) when all
    files share size and kind, else a list of per-file tensors in the files' order; status: int32 [F]."""
    single = isinstance(files, (bytes, bytearray, memoryview))
    files = [files] if single else list(files)
    out, status, whole = _decode_groups(files, _names(files, names), channels, first_channel, device)
    if whole is not None:
        return whole
    return out, torch.stack(status)


def decode(files, channels="bgr", first_channel=False, device=None, names=None):
    """One `bytes` -> a uint8 device tensor [H, W, 3] in B, G, R order (channels="rgb": R, G, B; "native": the file's own channels;
    first_channel=True: [H, W]).  A list -> [F, ...] when sizes and kinds agree, else a list of tensors.  An unsupported or corrupt file
    raises ValueError naming the file and the reason (one copy of the status words back to the host)."""
    single = isinstance(files, (bytes, bytearray, memoryview))
    lst = [files] if single else list(files)
    nm = _names(lst, names)
    px, status = decode_device(lst, channels, first_channel, device, nm)
    for k, st in enumerate(status.cpu().tolist()):
        if st:
            raise ValueError(f"png.decode: {nm[k]}: corrupt stream ({_lib.png_status_text(st)})")
    return px[0] if single else px


def imread_batch(paths, channels="bgr", first_channel=False, device=None):
    """the files at `paths` -> as decode() of their bytes"""
    data = []
    for p in paths:
        if str(p).lower().endswith((".jpg", ".jpeg")):
            raise ValueError(f"png.imread: {p}: a .jpg path - dsnerf_amd.jpeg.imread reads those")
        with open(p, "rb") as f:
            data.append(f.read())
    return decode(data, channels=channels, first_channel=first_channel, device=device, names=[str(p) for p in paths])


def imread(path, channels="bgr", first_channel=False, device=None):
    """cv2.imread(path)'s shape for a .png: uint8 [H, W, 3] in B, G, R order, on the device; first_channel=True: its [..., 0]"""
    return imread_batch([path], channels, first_channel, device)[0]
