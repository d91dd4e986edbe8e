"""PNG decoding on the device: the datasets' label masks (mask_cihp/....png - cv2.imread at dataloader/zju_mocap_dataset.py:197 and
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
import torch

from . import _lib

STATUS_NAMES = _lib.PNG_STATUS_NAMES


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
