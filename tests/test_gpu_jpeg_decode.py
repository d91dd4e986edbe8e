"""Baseline JPEG decoding on the device (dsn_jpegd_*, dsn_jpeg_decode, dsnerf_amd.jpeg.decode) against the numpy restatement of the rule
(tests/jpeg_decode_restate.py, which test_jpeg_decode_host.py pins to Pillow's pixels): pixels, coefficients as int16 words, status
words and synchronisation rounds are EQUAL, on outputs and workspaces pre-filled with 0xFF (DSN_POISON_SCRATCH), at sizes on and off
the 8- and 16-pixel grids, in the three sampling modes, with Annex K's and with optimised Huffman tables, at 128 and 1024 bits per
subsequence.  The files are written by the restatements (jpeg_restate.encode, jpeg_decode_restate.optimised_file): no Pillow needed.

The full product of quality x content x tables runs up to 37 x 53; 130 x 70 takes five and 256 x 256 three of its cases (the numpy
decoder needs about two microseconds per symbol), as test_gpu_jpeg.py thins the encoder's list at these sizes."""
import os

import numpy as np
import pytest
import torch

import jpeg_decode_restate as JD
import jpeg_restate as JR
from helpers import ROOT, load

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 3), (3, 2), (5, 4), (4, 5), (1, 6), (6, 1), (9, 5), (16, 16), (17, 33), (37, 53), (130, 70), (256, 256)]
SUBS = ["420", "444", "gray"]
QUALITIES = [1, 50, 95, 100]
KINDS = ["noise", "smooth", "constant"]


@pytest.fixture(scope="module")
def L():
    import dsnerf_amd
    return dsnerf_amd._lib


@pytest.fixture(scope="module")
def J():
    import dsnerf_amd
    return dsnerf_amd.jpeg


@pytest.fixture(autouse=True)
def poisoned_outputs(monkeypatch):
    monkeypatch.setenv("DSN_POISON_SCRATCH", "1")          # every output tensor and workspace starts as 0xFF bytes


def contents(H, W, C, seed):
    """noise, smooth and constant uint8 frames {kind: [H, W, C]}"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    smooth = np.stack([(128 + 100 * np.sin(x / 9.0 + k) * np.cos(y / 7.0 + 0.3 * k)).astype(np.uint8) for k in range(C)], -1)
    const = np.empty((H, W, C), np.uint8)
    const[...] = np.array([77, 130, 200])[:C]
    return {"noise": rng.integers(0, 256, (H, W, C), dtype=np.uint8), "smooth": smooth, "constant": const}


def make_file(img, q, sub, optimised):
    """the restatement encoder's file for `img` (R, G, B), with Annex K's tables or with tables made for its own symbols"""
    if not optimised:
        return JR.encode(img, q, sub, "rgb")[0]
    coef, _ = JR.coefficients(img, q, sub, "rgb")
    H, W = img.shape[:2]
    return JD.optimised_file(coef, H, W, JR.mode_of(sub, img.shape[2] if img.ndim == 3 else 1), q)


_expected = {}


def expected(data, B):
    """(coef int16 [blocks, 64], status, rounds, info) of the restatement, computed once per (file, B)"""
    key = (data, B)
    if key not in _expected:
        info = JD.parse(data)
        _expected[key] = JD.coefficients(data, B, info=info) + (info,)
    return _expected[key]


def batch_of(L, files):
    descs = []
    for f in files:
        d, st = L.jpeg_parse(f)
        assert st == 0, L.JPEGD_REASONS[st]
        descs.append(d)
    return L.JpegdBatch(files, descs)


def check_batch(L, files, B, what, gray_too=False):
    """one dsn_jpeg_decode call per channel order over `files` against the restatement: pixels, coef words, status, rounds"""
    batch = batch_of(L, files)
    want = [expected(f, B) for f in files]
    for rgb in (False, True):
        ws = batch.workspace()
        out, status, rounds, host = L.jpeg_decode(batch, B, rgb=rgb, workspace=ws)
        coef = L.jpegd_workspace_coef(batch, ws).cpu().numpy()
        px = out.cpu().numpy()
        assert status.cpu().tolist() == [w[1] for w in want], (what, rgb, status.cpu().tolist(), [w[1] for w in want])
        assert rounds.cpu().tolist() == [w[2] for w in want], (what, rgb, rounds.cpu().tolist(), [w[2] for w in want])
        for f, (c, st, rd, info) in enumerate(want):
            assert np.array_equal(coef[f].view(np.uint16), c.view(np.uint16)), (what, f, "coef")
            ref = JD.pixels(c, info, "rgb" if rgb else "bgr", status=st)
            assert np.array_equal(px[f], ref), (what, f, rgb, int((px[f] != ref).sum()))
    if gray_too:
        out, status, rounds, host = L.jpeg_decode(batch, B, gray=True)
        for f, (c, st, rd, info) in enumerate(want):
            assert np.array_equal(out[f].cpu().numpy(), JD.pixels(c, info, gray=True, status=st)), (what, f, "gray")


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("H,W", SIZES)
def test_decode_is_the_restatement(L, H, W, sub):
    C = 1 if sub == "gray" else 3
    imgs = contents(H, W, C, H * 1000 + W)
    if H * W <= 37 * 53:
        cases = [(q, k, o) for q in QUALITIES for k in KINDS for o in (False, True)]
    elif H * W <= 130 * 70:
        cases = [(95, "noise", False), (50, "smooth", True), (1, "constant", False), (100, "smooth", True), (95, "noise", True)]
    else:
        cases = [(95, "smooth", False), (50, "noise", True), (1, "constant", False)]
    files = [make_file(imgs[k][..., 0] if C == 1 else imgs[k], q, sub, o) for q, k, o in cases]
    for B in (128, 1024):
        check_batch(L, files, B, f"{H}x{W} {sub} B{B}", gray_too=(C == 1 and B == 128))
    assert all(expected(f, 128)[1] == 0 for f in files)          # every one of these files is sound


def test_decode_is_pixels_of_coefficients_of_sync(L):
    for sub, (H, W) in (("420", (37, 53)), ("444", (40, 48)), ("gray", (63, 65))):
        C = 1 if sub == "gray" else 3
        imgs = contents(H, W, C, 11)
        files = [make_file(imgs[k][..., 0] if C == 1 else imgs[k], q, sub, o) for k, q, o in (("noise", 90, False), ("smooth", 30, True))]
        batch = batch_of(L, files)
        for B in (128, 1024):
            out, status, rounds, host = L.jpeg_decode(batch, B)
            ws = batch.workspace()
            n = 0
            while True:
                conv, rnd = L.jpegd_sync(batch, ws, B, restart=(n == 0), rounds=L.JPEGD_ROUNDS)
                n += 1
                if bool(conv.cpu().all()):
                    break
            coef, st = L.jpegd_coefficients(batch, ws, B)
            px = L.jpegd_pixels(batch, coef, st, ws)
            assert torch.equal(px, out) and torch.equal(st, status) and torch.equal(rnd, rounds), (sub, B)
            assert np.array_equal(coef.cpu().numpy(), np.stack([expected(f, B)[0] for f in files]))


def test_one_round_per_call_and_rounds_after_convergence(L):
    """one round per dsn_jpegd_sync call until every frame has converged gives the bits of many rounds at once; further rounds change
    neither the counters nor the state"""
    imgs = contents(37, 53, 3, 5)
    files = [make_file(imgs["noise"], 100, "444", False), make_file(imgs["noise"], 75, "444", True)]
    batch = batch_of(L, files)
    B = 128
    want = [expected(f, B) for f in files]
    assert max(w[2] for w in want) > 2 * L.JPEGD_ROUNDS          # the noise frame at quality 100 keeps the rounds going
    ws1, ws2 = batch.workspace(), batch.workspace()
    calls = 0
    while True:
        conv, rnd = L.jpegd_sync(batch, ws1, B, restart=(calls == 0), rounds=1)
        calls += 1
        if bool(conv.cpu().all()):
            break
    assert calls == max(w[2] for w in want) and rnd.cpu().tolist() == [w[2] for w in want]
    conv2, rnd2 = L.jpegd_sync(batch, ws2, B, restart=True, rounds=calls + 7)
    assert torch.equal(rnd, rnd2) and bool(conv2.cpu().all())
    a, b = L.jpegd_coefficients(batch, ws1, B), L.jpegd_coefficients(batch, ws2, B)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    state = ws1.clone()
    conv3, rnd3 = L.jpegd_sync(batch, ws1, B, restart=False, rounds=5)
    assert torch.equal(rnd3, rnd) and torch.equal(ws1, state)
    c = L.jpegd_coefficients(batch, ws1, B)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    assert np.array_equal(a[0].cpu().numpy(), np.stack([w[0] for w in want]))


def test_batches_equal_single_calls(L):
    """F = 1, 2, 3, 5 and a permuted batch give each frame the bits of its own call; scans more than 4 x apart in length and a
    different set of tables in every frame"""
    H, W = 37, 53
    c = contents(H, W, 3, 21)
    files = [make_file(c["noise"], 95, "420", False), make_file(c["constant"], 95, "420", True), make_file(c["smooth"], 50, "420", True),
             make_file(c["noise"][::-1].copy(), 20, "420", False), make_file(c["constant"], 10, "420", False)]
    scans = [JD.parse(f)["scan_length"] for f in files]
    assert max(scans) > 4 * min(scans)
    single = []
    for f in files:
        b = batch_of(L, [f])
        out, st, rd, host = L.jpeg_decode(b, 128)
        single.append((out[0].clone(), int(host[0, 0]), int(host[1, 0])))
        c0, s0, r0, info = expected(f, 128)
        assert np.array_equal(out[0].cpu().numpy(), JD.pixels(c0, info)) and (s0, r0) == single[-1][1:]
    for order in ([0], [0, 1], [0, 1, 2], [0, 1, 2, 3, 4], [4, 2, 0, 3, 1]):
        out, st, rd, host = L.jpeg_decode(batch_of(L, [files[k] for k in order]), 128)
        for j, k in enumerate(order):
            assert torch.equal(out[j], single[k][0]) and (int(host[0, j]), int(host[1, j])) == single[k][1:], (order, j)


def test_truncated_scan_in_the_middle_of_the_buffer(L):
    """a frame whose bytes end early - its descriptor still promises the whole scan, and the next frame's bytes follow it in the
    buffer - is CORRUPT and all zeros; its neighbours keep their bits.  The same for a scan with its middle cut out (EOI in place)."""
    H, W = 40, 48
    c = contents(H, W, 3, 31)
    files = [make_file(c["noise"], 90, "444", False), make_file(c["smooth"], 90, "444", False), make_file(c["noise"][::-1].copy(), 90, "444", True)]
    good = L.jpeg_decode(batch_of(L, files), 128)[0]
    descs = [L.jpeg_parse(f)[0] for f in files]
    cut = files[1][:descs[1].scan_offset + descs[1].scan_length // 2]          # no EOI, half the scan: the descriptor is the whole file's
    out, st, rd, host = L.jpeg_decode(L.JpegdBatch([files[0], cut, files[2]], descs), 128)
    assert int(host[0, 0]) == 0 and int(host[0, 2]) == 0
    assert int(host[0, 1]) & L.JPEGD_CORRUPT and int(host[0, 1]) & L.JPEGD_COUNT
    assert torch.equal(out[0], good[0]) and torch.equal(out[2], good[2]) and not bool(out[1].any())
    i = JD.parse(files[1])
    a, n = i["scan_offset"], i["scan_length"]
    holed = files[1][:a + n // 3] + files[1][a + 2 * n // 3:]
    for B in (128, 1024):
        want = expected(holed, B)
        assert want[1] & JD.CORRUPT
        out, st, rd, host = L.jpeg_decode(batch_of(L, [files[0], holed, files[2]]), B)
        assert host[0].tolist() == [0, want[1], 0] and int(host[1, 1]) == want[2]
        assert torch.equal(out[0], good[0]) and torch.equal(out[2], good[2]) and not bool(out[1].any())


def test_marker_in_the_scan(L, J):
    H, W = 37, 53
    f = make_file(contents(H, W, 3, 41)["smooth"], 90, "420", False)
    i = JD.parse(f)
    at = i["scan_offset"] + i["scan_length"] // 2
    bad = f[:at] + b"\xff\xd0" + f[at + 2:]
    want = expected(bad, 128)
    assert want[1] & JD.MARKER and want[1] & JD.CORRUPT
    out, st, rd, host = L.jpeg_decode(batch_of(L, [f, bad]), 128)
    assert host[0].tolist() == [0, want[1]] and not bool(out[1].any()) and bool(out[0].any())
    with pytest.raises(ValueError, match="marker"):
        J.decode([f, bad], names=["good.jpg", "bad.jpg"])


def test_repeated_and_unpoisoned_calls_have_the_same_bits(L, monkeypatch):
    c = contents(63, 65, 3, 41)
    batch = batch_of(L, [make_file(c[k], 75, "420", k == "smooth") for k in KINDS])
    a = L.jpeg_decode(batch, 128)
    b = L.jpeg_decode(batch, 128)
    monkeypatch.delenv("DSN_POISON_SCRATCH")
    d = L.jpeg_decode(batch, 128)
    for other in (b, d):
        assert all(torch.equal(p, q) for p, q in zip(a[:3], other[:3]))


def test_module_surface(J, tmp_path):
    """one file and lists, mixed sizes and modes grouped, grey files, imread, refusals that name the file and the reason"""
    c = contents(37, 53, 3, 51)
    small = contents(9, 5, 3, 52)
    f = [make_file(c["noise"], 95, "420", False), make_file(c["smooth"], 60, "420", True), make_file(small["noise"], 95, "444", False),
         make_file(c["noise"][..., 0], 95, "gray", False)]
    ref = [JD.decode(x)[0] for x in f]
    one = J.decode(f[0])
    assert one.is_cuda and one.dtype == torch.uint8 and np.array_equal(one.cpu().numpy(), ref[0])
    stack = J.decode(f[:2])
    assert tuple(stack.shape) == (2, 37, 53, 3) and np.array_equal(stack.cpu().numpy(), np.stack(ref[:2]))
    mixed = J.decode(f)
    assert isinstance(mixed, list) and all(np.array_equal(m.cpu().numpy(), r) for m, r in zip(mixed, ref))
    assert np.array_equal(J.decode(f[0], channels="rgb").cpu().numpy(), ref[0][..., ::-1])
    assert np.array_equal(J.decode(f[3], gray=True).cpu().numpy(), ref[3][..., 0])
    px, status, rounds = J.decode_device(f[:2], subseq_bits=256)
    assert px.is_cuda and status.tolist() == [0, 0] and rounds.tolist() == [JD.coefficients(x, 256)[2] for x in f[:2]]
    p = tmp_path / "a.jpg"
    p.write_bytes(f[1])
    assert np.array_equal(J.imread(str(p)).cpu().numpy(), ref[1])
    assert np.array_equal(J.imread_batch([str(p), str(p)]).cpu().numpy(), np.stack([ref[1]] * 2))
    g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_decode_pillow.npz"))
    for k in g["refused"]:
        name, reason = str(k).split()
        with pytest.raises(ValueError, match=f"x.jpg.*{reason}"):
            J.decode([f[0], g[f"refused_{name}"].tobytes()], names=["ok.jpg", "x.jpg"])
    with pytest.raises(ValueError):
        J.decode(f[0], channels="gbr")
    with pytest.raises(ValueError):
        J.decode(f[0], gray=True)
    with pytest.raises(ValueError):
        J.decode(f[0], subseq_bits=100)


def test_fixture_pillow_pixels(J):
    """the files Pillow (libjpeg-turbo) wrote and the pixels it decoded from them, where Pillow itself may not import"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_decode_pillow.npz"))
    files = [g[f"jpg_{str(line).split()[0]}"].tobytes() for line in g["meta"]]
    got = J.decode(files, channels="rgb")
    for line, px in zip(g["meta"], got):
        k = str(line).split()[0]
        want = g[f"px_{k}"]
        want = np.repeat(want[..., None], 3, 2) if want.ndim == 2 else want
        assert np.array_equal(px.cpu().numpy(), want), line


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def renderer():
    from cases import make_renderer
    g = load("small_eval")
    r = make_renderer(g, "small_eval")
    r.eval()
    return g, r


def view_batch():
    from cases import make_batch
    gv = load("small_view")
    Hv, Wv = int(gv["H"]), int(gv["W"])
    b = make_batch(gv)
    b["img"] = torch.zeros(1, Hv, Wv, 3, dtype=torch.float64)
    b["mask_at_box"] = torch.from_numpy(gv["mask_at_box"])[None]
    return b, Hv, Wv


def test_decode_of_encode(J):
    """jpeg.decode(jpeg.encode(frame)) is the restatement's decode of the restatement's file"""
    c = contents(63, 65, 3, 61)
    for sub, q in (("420", 95), ("444", 40)):
        frames = np.stack([c[k] for k in KINDS])
        files = J.encode(torch.from_numpy(frames).cuda(), quality=q, subsampling=sub)
        assert files == [JR.encode(x, q, sub)[0] for x in frames]
        got = J.decode(files)
        assert np.array_equal(got.cpu().numpy(), np.stack([JD.decode(x)[0] for x in files]))


def test_rendered_512_frame_prepare_and_render_view(J, renderer):
    """a rendered frame brought to 512 x 512, encoded and decoded on the device: the restatement's pixels, and Pillow's where Pillow
    imports; imageprep.prepare_zju takes the decoded tensor as it is and gives, key for key, what it gives for the uploaded reference
    array, and sample_batch runs on it; render_view is bit-identical before and after"""
    import dsnerf_amd
    g, r = renderer
    b, Hv, Wv = view_batch()
    host = lambda: {k: v.clone() for k, v in r.render_view(b).items() if torch.is_tensor(v)}          # noqa: E731
    before = host()
    small = r.render_view(b, device_output=True)["coarse_color"]
    big = torch.nn.functional.interpolate(small.permute(2, 0, 1)[None].float(), size=(512, 512), mode="bilinear")[0].permute(1, 2, 0)
    big = (big + 0.1 * torch.rand(512, 512, 3, device=big.device, generator=torch.Generator(big.device).manual_seed(3))).contiguous()
    data = J.encode(big, quality=95)[0]
    frame = J.decode(data)
    ref, st, _ = JD.decode(data)
    assert st == 0 and tuple(frame.shape) == (512, 512, 3) and np.array_equal(frame.cpu().numpy(), ref)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        import io
        assert np.array_equal(ref[..., ::-1], np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))
    H = W = 512
    K = np.array([[0.9 * W + 0.37, 0.0, W / 2 - 0.3], [0.0, 0.92 * W + 0.11, H / 2 + 0.2], [0.0, 0.0, 1.0]])
    D = np.array([-0.3, 0.12, 1.5e-3, -2e-3, 0.03])
    cihp = np.zeros((H, W), np.uint8)
    cihp[100:420, 150:380] = 3
    P = dsnerf_amd.imageprep
    mine = P.prepare_zju(frame, torch.from_numpy(cihp).cuda(), K, D, ratio=0.5)
    theirs = P.prepare_zju(torch.from_numpy(ref).cuda(), torch.from_numpy(cihp).cuda(), K, D, ratio=0.5)
    assert mine.keys() == theirs.keys()
    for k in mine:
        if torch.is_tensor(mine[k]):
            assert torch.equal(mine[k], theirs[k]), k
        else:
            assert np.array_equal(np.asarray(mine[k]), np.asarray(theirs[k])), k
    xyz = g["xyz"]
    lo, hi = xyz.min(0) - 0.05, xyz.max(0) + 0.05
    R, T = np.eye(3), np.array([0.0, 0.0, 3.0]) - (lo + hi) / 2
    batch = r.sample_batch(mine["img"], mine["K"], R, T, np.stack([lo, hi]).astype(np.float64), mine["msk_cihp"], 64, 7,
                           occupancy_from=mine["msk_fg"], check=False)
    assert batch["rgb"].is_cuda and batch["rgb"].shape[-1] == 3
    after = host()
    assert before.keys() == after.keys()
    for k in before:
        assert torch.equal(before[k].contiguous().view(torch.uint8), after[k].contiguous().view(torch.uint8)), k
