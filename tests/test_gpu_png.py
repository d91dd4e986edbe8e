"""PNG decoding on the device (dsn_png_decode, dsnerf_amd.png) against the numpy restatement of the rule (tests/png_decode_restate.py,
which test_png_host.py pins to zlib.decompress and to Pillow's pixels): the gathered stream, the inflated bytes, the unfiltered rows,
the pixels in the three channel settings and with first_channel, and the status words are EQUAL, on outputs and workspaces
pre-filled with 0xFF (DSN_POISON_SCRATCH).  The files are those of tests/golden/png_pillow.npz: neither Pillow nor zlib's inflate is
needed for the comparison.  The 1024 x 1024 label maps are compared with the recorded Pillow pixels and with zlib.decompress, not
with the (slow) restatement.

Every corrupt file here is an input a correct decoder flags: the checks are that the call returns with the file's status bit set, a
zero frame, its neighbours' bits intact and the guard bands around every buffer untouched."""
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import dsnerf_amd.png  # noqa: F401  (every test here is about this module)
import png_decode_restate as PR
from helpers import ROOT, load

pytestmark = pytest.mark.gpu

GUARD = 4096


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(ROOT, "tests", "golden", "png_pillow.npz"))


@pytest.fixture(scope="module")
def L():
    import dsnerf_amd
    import dsnerf_amd.png  # noqa: F401
    return dsnerf_amd._lib


@pytest.fixture(scope="module")
def P():
    import dsnerf_amd
    return dsnerf_amd.png


@pytest.fixture(autouse=True)
def poisoned_outputs(monkeypatch):
    monkeypatch.setenv("DSN_POISON_SCRATCH", "1")          # every output tensor and workspace starts as 0xFF bytes


_restated = {}


def restated(data):
    """the restatement's stages of one file, computed once and shared"""
    if data not in _restated:
        _restated[data] = PR.stages(data)
    return _restated[data]


def small_files(G):
    """{(W, H, bits, ctype): [(key, bytes)]} of the fixture's files at or below 256 x 256, and of the two wide ones made for distances of
    8192 and 32768 (six rows each): everything but the three 1024 x 1024 label maps"""
    groups = {}
    for line in G["meta"]:
        k, _, W, H, bits, ctype = str(line).split()
        if int(W) * int(H) <= 256 * 256 or int(H) <= 6:
            groups.setdefault((int(W), int(H), int(bits), int(ctype)), []).append((k, G[f"png_{k}"].tobytes()))
    return groups


def batch_of(L, files):
    descs, segs = [], []
    for f in files:
        d, s, st = L.png_parse(f)
        assert st == 0, L.PNG_REASONS[st]
        descs.append(d)
        segs.append(s)
    return L.PngBatch(files, descs, segs)


def check_stages(L, files, what):
    """one dsn_png_decode call over `files`: every stage's buffer against the restatement; the other channel settings from the pixel stage
    alone on the same workspace"""
    batch = batch_of(L, files)
    want = [restated(f) for f in files]
    ws = batch.workspace()
    out, status = L.png_decode(batch, "bgr", workspace=ws)
    meta, streams, raw, rows = (t.cpu().numpy() for t in batch.views(ws))
    assert status.cpu().tolist() == [w["status"] for w in want], (what, status.cpu().tolist())
    H, rb, need = batch.H, batch.row_bytes, batch.raw_bytes
    for f, w in enumerate(want):
        z = np.frombuffer(w["stream"], np.uint8)
        assert np.array_equal(streams[f, :len(z)], z) and not streams[f, len(z):].any(), (what, f, "stream")
        assert int(meta[f, 0]) == len(w["raw"]) and int(meta[f, 1]) == w["status"], (what, f, meta[f].tolist())
        assert np.array_equal(raw[f, :len(w["raw"])], np.frombuffer(w["raw"], np.uint8)), (what, f, "inflated bytes")
        assert (raw[f, len(w["raw"]):] == 255).all(), (what, f, "bytes behind the inflated data were written")
        if w["adler"] is not None:
            assert int(meta[f, 2]) & 0xFFFFFFFF == w["stored"] and int(meta[f, 3]) & 0xFFFFFFFF == w["adler"], (what, f, "adler")
        assert int(meta[f, 4]) == w["endbit"], (what, f, "end bit")
        if w["rows"] is not None:
            assert np.array_equal(rows[f, :H * rb].reshape(H, rb), w["rows"]), (what, f, "rows")
            assert (rows[f, H * rb:] == 255).all(), (what, f, "bytes behind the rows were written")
    for channels in ("bgr", "rgb", "native"):
        for first in (False, True):
            if channels == "bgr" and not first:
                px = out
            else:
                px, st2 = L.png_decode(batch, channels, first, stages=L.PNG_PIXELS, workspace=ws)
                assert torch.equal(st2, status)
            px = px.cpu().numpy()
            for f, w in enumerate(want):
                r = w["rows"] if w["rows"] is not None else np.zeros((H, rb), np.uint8)
                ref = PR.pixels(r, w["info"], channels, first, w["status"])
                assert px[f].shape == ref.shape and np.array_equal(px[f], ref), (what, f, channels, first, int((px[f] != ref).sum()))
    return out, status


def test_every_stage_is_the_restatement(G, L):
    groups = small_files(G)
    assert len(groups) > 100
    n = 0
    for geo, items in groups.items():
        check_stages(L, [d for _, d in items], f"{geo} {[k for k, _ in items]}")
        n += len(items)
    assert n == len(G["meta"]) - 3


def test_label_maps_1024(G, L, P):
    """the masks' own shape: Pillow's recorded pixels and zlib.decompress, single and as a batch of four"""
    for name in ("L", "P", "RGB"):
        k = f"mask_{name}_1024"
        data = G[f"png_{k}"].tobytes()
        batch = batch_of(L, [data] * 4)
        ws = batch.workspace()
        out, status = L.png_decode(batch, "native", workspace=ws)
        assert status.cpu().tolist() == [0] * 4
        meta, streams, raw, rows = batch.views(ws)
        info = PR.parse(data)
        inflated = zlib.decompress(PR.gather(data, info))
        want = G[f"px_{k}"]
        want = want[..., None] if want.ndim == 2 else want
        for f in range(4):
            assert raw[f, :len(inflated)].cpu().numpy().tobytes() == inflated, (k, f)
            assert np.array_equal(out[f].cpu().numpy(), want), (k, f)
        rgb = G[f"rgb_{k}"] if f"rgb_{k}" in G.files else np.repeat(want[..., :1], 3, 2) if want.shape[2] == 1 else want
        assert np.array_equal(P.decode(data).cpu().numpy(), rgb[..., ::-1]), k
        assert np.array_equal(P.decode(data, first_channel=True).cpu().numpy(), rgb[..., 2]), k


def test_batches_equal_single_calls_in_any_order(G, L, monkeypatch):
    """a batch of F files = F single calls, in any order; the same call twice = the same bits, with and without poisoned scratch"""
    keys = [str(m).split()[0] for m in G["meta"] if str(m).split()[2:] == ["130", "70", "8", "6"]]
    assert len(keys) >= 6
    files = [G[f"png_{k}"].tobytes() for k in keys]
    single = []
    for f in files:
        o, s = L.png_decode(batch_of(L, [f]), "native")
        assert np.array_equal(o[0].cpu().numpy(), PR.pixels(restated(f)["rows"], restated(f)["info"], "native"))
        single.append((o[0].clone(), int(s[0])))
    n = len(files)
    for order in (list(range(n)), list(range(n))[::-1], [3, 0, 5, 1], [2, 2, 2], [4]):
        batch = batch_of(L, [files[k] for k in order])
        a = L.png_decode(batch, "native")
        b = L.png_decode(batch, "native")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for j, k in enumerate(order):
            assert torch.equal(a[0][j], single[k][0]) and int(a[1][j]) == single[k][1], (order, j)
    batch = batch_of(L, files)
    a = L.png_decode(batch, "bgr")
    monkeypatch.delenv("DSN_POISON_SCRATCH")
    b = L.png_decode(batch, "bgr")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def guarded(n, dtype=torch.uint8):
    """a tensor of n elements between two guard bands of 0xA5 bytes: (the whole allocation, the view between)"""
    size = n * torch.empty(0, dtype=dtype).element_size()
    whole = torch.full((size + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    whole[GUARD:GUARD + size] = 0xFF
    return whole, whole[GUARD:GUARD + size].view(dtype)


def guards_intact(whole):
    return bool((whole[:GUARD] == 0xA5).all()) and bool((whole[-GUARD:] == 0xA5).all())


def test_corrupt_files_are_flagged_and_confined(G, L, P):
    """every corrupt file between two sound ones of its size: its status bit, a zero frame, the neighbours' bits, the guard bands around
    the output, the status words and the workspace, and inside the workspace nothing written behind a file's own buffers"""
    by_geo = {}
    for line in G["corrupt"]:
        k, expect, _ = str(line).split()
        data = G[f"bad_{k}"].tobytes()
        i = PR.parse(data)
        by_geo.setdefault((i["W"], i["H"], i["bits"], i["ctype"]), []).append((k, expect, data))
    assert sum(len(v) for v in by_geo.values()) == len(G["corrupt"]) > 15
    for (W, H, bits, ctype), items in by_geo.items():
        good = G["bad_trailing_garbage"].tobytes() if (W, H, bits, ctype) == (37, 11, 8, 2) else None
        files = [d for _, _, d in items]
        if good is not None:
            files = [good] + files + [good]
        batch = batch_of(L, files)
        F = len(files)
        w_all, ws = guarded(batch.workspace_bytes)
        o_all, out = guarded(F * H * W * 3)
        s_all, status = guarded(F, torch.int32)
        L.png_decode(batch, "bgr", workspace=ws, out=out.view(F, H, W, 3), status=status)
        torch.cuda.synchronize()
        assert guards_intact(w_all) and guards_intact(o_all) and guards_intact(s_all)
        st = status.cpu().tolist()
        px = out.view(F, H, W, 3).cpu().numpy()
        meta, streams, raw, rows = (t.cpu().numpy() for t in batch.views(ws))
        off = 1 if good is not None else 0
        for j, (k, expect, data) in enumerate(items):
            w = restated(data)
            f = j + off
            assert st[f] == w["status"] == (PR.STATUS_BITS[expect] if expect != "ok" else 0), (k, expect, st[f])
            assert int(meta[f, 0]) == len(w["raw"]) <= batch.raw_bytes, k
            assert (raw[f, len(w["raw"]):] == 255).all(), (k, "bytes behind the inflated data were written")
            assert np.array_equal(raw[f, :len(w["raw"])], np.frombuffer(w["raw"], np.uint8)), k
            if expect != "ok":
                assert not px[f].any(), k
                if expect not in ("filter",):
                    assert (rows[f] == 255).all(), (k, "rows of a frame that has a status were written")
        if good is not None:
            ref = PR.decode(good)[0]
            assert st[0] == st[-1] == 0 and np.array_equal(px[0], ref) and np.array_equal(px[-1], ref)
    # the module: decode raises and names the file and the reason; decode_device does not
    bad = G["bad_adler"].tobytes()
    ok = G["bad_trailing_garbage"].tobytes()
    with pytest.raises(ValueError, match="b.png.*Adler"):
        P.decode([ok, bad], names=["a.png", "b.png"])
    px, st = P.decode_device([ok, bad])
    assert px.is_cuda and st.is_cuda and st.cpu().tolist() == [0, PR.ADLER] and not bool(px[1].any()) and bool(px[0].any())


def test_module_surface(G, P, tmp_path):
    """one file and lists, mixed sizes and kinds grouped, channel settings, first_channel, imread, refusals that name file and reason"""
    f = [G[f"png_{k}"].tobytes() for k in ("pil_RGB_130x70_l6", "pil_RGB_130x70_l0", "pil_P_65x5", "hand_L2_9x5", "pil_RGBA_9x5", "pil_LA_9x5")]
    ref = [PR.decode(x)[0] for x in f]
    one = P.decode(f[0])
    assert one.is_cuda and one.dtype == torch.uint8 and np.array_equal(one.cpu().numpy(), ref[0])
    stack = P.decode(f[:2])
    assert tuple(stack.shape) == (2, 70, 130, 3) and np.array_equal(stack.cpu().numpy(), np.stack(ref[:2]))
    mixed = P.decode(f)
    assert isinstance(mixed, list) and all(np.array_equal(m.cpu().numpy(), r) for m, r in zip(mixed, ref))
    for x in f:
        for ch in ("rgb", "native"):
            for first in (False, True):
                assert np.array_equal(P.decode(x, channels=ch, first_channel=first).cpu().numpy(), PR.decode(x, ch, first)[0])
    assert tuple(P.decode(f[4], channels="native").shape) == (5, 9, 4) and tuple(P.decode(f[5], channels="native").shape) == (5, 9, 2)
    assert tuple(P.decode(f[2], first_channel=True).shape) == (5, 65)
    px, status = P.decode_device(f[:2])
    assert px.is_cuda and status.is_cuda and status.cpu().tolist() == [0, 0]
    p = tmp_path / "a.png"
    p.write_bytes(f[1])
    assert np.array_equal(P.imread(str(p)).cpu().numpy(), ref[1])
    assert np.array_equal(P.imread(str(p), first_channel=True).cpu().numpy(), ref[1][..., 0])
    assert np.array_equal(P.imread_batch([str(p), str(p)]).cpu().numpy(), np.stack([ref[1]] * 2))
    for line in G["refused"]:
        k, reason = str(line).split()
        with pytest.raises(ValueError, match=f"x.png.*{reason}"):
            P.decode([f[0], G[f"ref_{k}"].tobytes()], names=["ok.png", "x.png"])
    with pytest.raises(ValueError):
        P.decode(f[0], channels="gbr")
    with pytest.raises(ValueError):
        P.decode([])


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def png_of(gray):
    """a grey 8-bit PNG of `gray` [H, W] by zlib.compress (filter 0 on every row)"""
    H, W = gray.shape
    raw = b"".join(b"\0" + gray[r].tobytes() for r in range(H))

    def chunk(t, b):
        return struct.pack(">I", len(b)) + t + b + struct.pack(">I", zlib.crc32(t + b))

    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 0, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b"")


@pytest.fixture(scope="module")
def renderer():
    from cases import make_renderer
    g = load("small_eval")
    r = make_renderer(g, "small_eval")
    r.eval()
    return g, r


def test_file_bytes_to_training_item(G, P, renderer, tmp_path):
    """prepare_zju(jpeg.imread(frame), png.imread(mask, first_channel=True), ...) = prepare_zju of the host-decoded arrays bit for bit, the
    same for prepare_h36m; render_view is bit-identical before and after the decodes"""
    import dsnerf_amd
    import jpeg_decode_restate as JD
    import jpeg_restate as JR
    from cases import make_batch
    g, r = renderer
    gv = load("small_view")
    b = make_batch(gv)
    b["img"] = torch.zeros(1, int(gv["H"]), int(gv["W"]), 3, dtype=torch.float64)
    b["mask_at_box"] = torch.from_numpy(gv["mask_at_box"])[None]
    host = lambda: {k: v.clone() for k, v in r.render_view(b).items() if torch.is_tensor(v)}          # noqa: E731
    before = host()
    H = W = 256
    y, x = np.mgrid[0:H, 0:W]
    frame = np.stack([(128 + 100 * np.sin(x / 9.0 + k) * np.cos(y / 7.0 + 0.3 * k)).astype(np.uint8) for k in range(3)], -1)
    labels = G["px_mask_L_1024"][300:300 + H, 200:200 + W].copy()
    assert len(np.unique(labels)) > 2
    jp, pp = tmp_path / "000000.jpg", tmp_path / "000000.png"
    jp.write_bytes(JR.encode(frame, 95, "420", "rgb")[0])
    pp.write_bytes(png_of(labels))
    img = dsnerf_amd.jpeg.imread(str(jp))
    msk = P.imread(str(pp), first_channel=True)
    assert msk.is_cuda and tuple(msk.shape) == (H, W) and np.array_equal(msk.cpu().numpy(), labels)
    img_host = JD.decode(jp.read_bytes())[0]
    assert np.array_equal(img.cpu().numpy(), img_host)
    K = np.array([[0.9 * W + 0.37, 0.0, W / 2 - 0.3], [0.0, 0.92 * W + 0.11, H / 2 + 0.2], [0.0, 0.0, 1.0]])
    D = np.array([-0.3, 0.12, 1.5e-3, -2e-3, 0.03])
    I = dsnerf_amd.imageprep
    for prep, kw in ((I.prepare_zju, {"ratio": 0.5}), (I.prepare_h36m, {"ratio": 1.0})):
        mine = prep(img, msk, K, D, **kw)
        theirs = prep(torch.from_numpy(img_host).cuda(), torch.from_numpy(labels).cuda(), K, D, **kw)
        assert mine.keys() == theirs.keys()
        for k in mine:
            if torch.is_tensor(mine[k]):
                assert torch.equal(mine[k], theirs[k]), (prep.__name__, k)
            else:
                assert np.array_equal(np.asarray(mine[k]), np.asarray(theirs[k])), (prep.__name__, k)
    after = host()
    assert before.keys() == after.keys()
    for k in before:
        assert torch.equal(before[k].contiguous().view(torch.uint8), after[k].contiguous().view(torch.uint8)), k
