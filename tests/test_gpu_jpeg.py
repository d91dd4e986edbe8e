"""Baseline JPEG on the device (dsn_jpeg_*, dsnerf_amd.jpeg, Renderer.save_views) against the numpy restatement of the rule
(tests/jpeg_restate.py, which test_jpeg_host.py pins to Pillow's bytes): files, lengths and status words are EQUAL, on outputs and
workspaces pre-filled with 0xFF (DSN_POISON_SCRATCH), at sizes on and off the 8- and 16-pixel grids, in all three sampling modes."""
import os

import numpy as np
import pytest
import torch

import jpeg_restate as JR
from helpers import ROOT, load

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (7, 5), (8, 8), (16, 16), (16, 17), (17, 9), (37, 53), (40, 48), (63, 65), (130, 70), (256, 256)]
SUBS = ["420", "444", "gray"]
QUALITIES = [1, 50, 95, 100]


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


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def contents(H, W, C, seed):
    """noise, smooth and constant uint8 frames [3, H, W, C]"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    smooth = np.stack([(128 + 100 * np.sin(x / 9.0 + k) * np.cos(y / 7.0 + 0.3 * k)).astype(np.uint8) for k in range(C)], -1)
    const = np.empty((H, W, C), np.uint8)
    const[...] = np.array([77, 130, 200])[:C]
    return np.stack([rng.integers(0, 256, (H, W, C), dtype=np.uint8), smooth, const])


def squeeze(stack, C):
    return stack[..., 0] if C == 1 else stack


def check(L, out, lengths, status, want, what):
    """rows of `out` against the restatement's (bytes, status) pairs; the bytes behind a file still 0xFF"""
    out, lengths, status = out.cpu().numpy(), lengths.cpu().numpy(), status.cpu().numpy()
    for f, (data, st) in enumerate(want):
        assert int(lengths[f]) == len(data), (what, f, int(lengths[f]), len(data))
        assert int(status[f]) == st, (what, f, int(status[f]), st)
        got = out[f, :len(data)].tobytes()
        if got != data:
            first = next(i for i in range(len(data)) if got[i] != data[i])
            raise AssertionError(f"{what}, frame {f}: first differing byte {first} of {len(data)}")
        assert (out[f, len(data):] == 0xFF).all(), (what, f, "bytes past the file were written")


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("H,W", SIZES)
def test_encode_is_the_restatement(L, H, W, sub):
    C = 1 if sub == "gray" else 3
    mode = JR.mode_of(sub, C)
    u8 = contents(H, W, C, H * 1000 + W)
    rng = np.random.default_rng(5)
    wild = (rng.random((H, W, C)) * 1.5 - 0.25).astype(np.float32)          # values outside [0, 1]
    wild.reshape(-1)[::7] = (np.arange(wild.size)[::7] % 256 + 0.5).astype(np.float32) / np.float32(255.0)      # near ties
    nan = (u8[0] / 255.0).astype(np.float32)
    nan.reshape(-1)[nan.size // 2] = np.nan
    nan.reshape(-1)[0] = np.inf
    f32 = np.concatenate([(u8 / 255.0).astype(np.float32), wild[None], nan[None]])
    for q in (QUALITIES if H * W <= 130 * 70 else [95]):
        for stack, rgb in ((u8, False), (f32, True)):
            want = [JR.encode(img, q, sub, "rgb" if rgb else "bgr") for img in stack]
            out, n, st = L.jpeg_encode(dev(squeeze(stack, C)), mode, q, rgb)
            check(L, out, n, st, want, f"{H}x{W} {sub} q{q} {stack.dtype}")
            if stack is f32:
                assert [w[1] for w in want] == [0, 0, 0, 0, JR.NONFINITE]          # the NaN frame alone carries the bit


@pytest.mark.parametrize("sub", SUBS)
def test_coefficients_are_the_restatement(L, sub):
    C = 1 if sub == "gray" else 3
    for H, W in [(1, 1), (17, 9), (37, 53), (63, 65), (130, 70)]:
        u8 = contents(H, W, C, 3)
        for q in (1, 50, 100):
            coef, st = L.jpeg_coefficients(dev(squeeze(u8, C)), JR.mode_of(sub, C), q)
            want = np.stack([JR.coefficients(img, q, sub)[0] for img in u8])
            assert coef.dtype == torch.int16 and tuple(coef.shape) == want.shape
            assert np.array_equal(coef.cpu().numpy(), want), (H, W, sub, q)
            assert st.cpu().tolist() == [0, 0, 0]


@pytest.mark.parametrize("name", sorted(JR.hand_made_scans()))
def test_scan_of_hand_made_coefficients(L, name):
    coef, mode, H, W = JR.hand_made_scans()[name]
    for q in (50, 100):
        out, n, st = L.jpeg_scan(dev(coef[None]), H, W, mode, q)
        check(L, out, n, st, [(JR.scan_file(coef, H, W, mode, q), 0)], name)


def test_encode_is_scan_of_coefficients(L):
    for sub, (H, W) in (("420", (37, 53)), ("444", (40, 48)), ("gray", (63, 65))):
        C = 1 if sub == "gray" else 3
        mode = JR.mode_of(sub, C)
        x = (contents(H, W, C, 11) / 255.0).astype(np.float32)
        x[0].reshape(-1)[5] = np.nan
        x = dev(squeeze(x, C))
        a = L.jpeg_encode(x, mode, 90)
        coef, st = L.jpeg_coefficients(x, mode, 90)
        b = L.jpeg_scan(coef, H, W, mode, 90, status_in=st)
        assert all(torch.equal(p, q) for p, q in zip(a, b))
        assert a[2].cpu().tolist() == [JR.NONFINITE, 0, 0]


def test_batches_equal_single_calls(L):
    """F = 1, 2, 3, 5 and a permuted batch give each frame the bytes of its own call; frames of very different lengths side by side"""
    H, W = 37, 53
    c = contents(H, W, 3, 21)
    frames = np.stack([c[0], c[2], c[1], c[0][::-1].copy(), c[2]])          # noise (long), constant (short), ...
    single = []
    for f in range(5):
        out, n, st = L.jpeg_encode(dev(frames[f:f + 1]), JR.M420, 95)
        single.append(out[0, :int(n[0])].cpu().numpy().tobytes())
    assert max(len(s) for s in single) - 623 > 4 * (min(len(s) for s in single) - 623)          # the scans' lengths differ by more than 4 x
    assert single == [JR.encode(f, 95, "420")[0] for f in frames]
    for order in ([0], [0, 1], [0, 1, 2], [0, 1, 2, 3, 4], [4, 2, 0, 3, 1]):
        out, n, st = L.jpeg_encode(dev(frames[order]), JR.M420, 95)
        check(L, out, n, st, [(single[k], 0) for k in order], f"batch {order}")


def test_more_scan_tiles_than_one_workgroup_holds(L):
    """143 x 143 grey blocks: 20 tiles of block lengths and 260 tiles of 0xFF counts, more than the 256 entries the workgroup that
    scans a frame's tile totals takes per trip; a noisy band keeps 0xFF bytes in play across many tiles"""
    H = W = 1144
    y, x = np.mgrid[0:H, 0:W]
    img = (128 + 100 * np.sin(x / 31.0) * np.cos(y / 23.0)).astype(np.uint8)
    img[300:420] = np.random.default_rng(9).integers(0, 256, (120, W), dtype=np.uint8)
    assert JR.n_blocks(H, W, JR.MGRAY) * 208 // 16 > 256 * 1024
    out, n, st = L.jpeg_encode(dev(img[None]), JR.MGRAY, 90)
    check(L, out, n, st, [JR.encode(img, 90, "gray")], "1144 x 1144 grey")


def test_capacity_one_byte_short(L):
    """a frame that needs one byte more than the capacity: OVERFLOW for it alone, the needed length reported, nothing written at or
    past the capacity (its row's last byte is the neighbour's first), the guard behind the buffer untouched"""
    H, W = 40, 48
    c = contents(H, W, 3, 31)
    frames = np.stack([c[2], c[0], c[2]])
    want = [JR.encode(f, 95, "444")[0] for f in frames]
    cap = len(want[1]) - 1
    assert len(want[0]) < cap
    big = torch.full((3 * cap + 256,), 0xAB, dtype=torch.uint8, device="cuda")
    out, n, st = L.jpeg_encode(dev(frames), JR.M444, 95, out=big[:3 * cap].view(3, cap))
    assert n.cpu().tolist() == [len(w) for w in want]
    assert st.cpu().tolist() == [0, JR.OVERFLOW, 0]
    got = big.cpu().numpy()
    assert (got[3 * cap:] == 0xAB).all()
    for f in (0, 2):
        row = got[f * cap:(f + 1) * cap]
        assert row[:len(want[f])].tobytes() == want[f] and (row[len(want[f]):] == 0xAB).all()
    assert got[cap:2 * cap].tobytes() == want[1][:cap]          # what fits is the file's beginning


def test_repeated_and_unpoisoned_calls_have_the_same_bytes(L, monkeypatch):
    x = dev(contents(63, 65, 3, 41))
    a = L.jpeg_encode(x, JR.M420, 75)
    b = L.jpeg_encode(x, JR.M420, 75)
    monkeypatch.delenv("DSN_POISON_SCRATCH")
    c = L.jpeg_encode(x, JR.M420, 75)
    n = a[1].cpu().tolist()
    for other in (b, c):
        assert torch.equal(a[1], other[1]) and torch.equal(a[2], other[2])
        assert all(torch.equal(a[0][f, :n[f]], other[0][f, :n[f]]) for f in range(3))


def test_fixture_pillow_bytes(J):
    """the bytes Pillow (libjpeg-turbo) wrote for the fixture's images, where Pillow itself may not import"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_pillow.npz"))
    for line in g["meta"]:
        k, H, W, sub, q, kind = str(line).split()
        got = J.encode(g[f"img_{k}"], quality=int(q), subsampling=sub, channels="rgb")
        assert got == [g[f"jpg_{k}"].tobytes()], line


def test_module_surface(J, tmp_path):
    """lists, [H, W, 1], non-contiguous and host inputs, float64; imwrite's params and extension check"""
    c = contents(37, 53, 3, 51)
    want = [JR.encode(f, 95, "420")[0] for f in c]
    assert J.encode([dev(f) for f in c]) == want
    assert J.encode(c) == want                                              # a host stack is uploaded
    wide = dev(np.concatenate([c, c], 2))
    assert J.encode(wide[:, :, :53]) == want                                # non-contiguous rows
    assert J.encode((c / 255.0).astype(np.float64)) == want                 # float64 is cast to float32
    grey = c[0, :, :, :1]
    assert J.encode(grey) == J.encode(grey[..., 0]) == [JR.encode(grey, 95, "gray")[0]]
    assert J.encode(c[0], quality=30, subsampling="444", channels="rgb") == [JR.encode(c[0], 30, "444", "rgb")[0]]
    buf, n, st = J.encode_device(dev(c))
    assert buf.is_cuda and n.is_cuda and st.is_cuda and n.cpu().tolist() == [len(w) for w in want]
    p = tmp_path / "a.jpg"
    assert J.imwrite(str(p), c[0].astype(np.float32) * np.float32(1.0), [J.IMWRITE_JPEG_QUALITY, 60]) is True
    assert p.read_bytes() == JR.encode(c[0], 60, "420")[0]
    lv = (np.random.default_rng(1).random((16, 17, 3)) * 300 - 20).astype(np.float32)          # cv2.imwrite(path, img * 255): levels as floats
    J.imwrite(str(p), torch.from_numpy(lv))
    assert p.read_bytes() == JR.encode(lv, 95, "420", scale=1.0)[0]
    with pytest.raises(ValueError, match="jpg"):
        J.imwrite(str(tmp_path / "a.png"), c[0])
    with pytest.raises(ValueError):
        J.encode(c[0], quality=0)
    with pytest.raises(ValueError):
        J.encode(c[0], channels="gbr")
    with pytest.raises(ValueError):
        J.encode([c[0], c[0][:8]])
    n = J.write_avi(str(tmp_path / "a.avi"), want, fps=25)
    assert n == 3 and (tmp_path / "a.avi").read_bytes()[:4] == b"RIFF"


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
    y, x = np.mgrid[0:Hv, 0:Wv]
    b["img"] = torch.from_numpy(np.stack([(x + k * y) % 17 / 16.0 for k in range(3)], -1))[None]          # float64 [1, H, W, 3]
    b["mask_at_box"] = torch.from_numpy(gv["mask_at_box"])[None]
    return b, Hv, Wv


def test_save_views_end_to_end(renderer, tmp_path):
    """render_view(device_output=True) -> save_views with and without gt, depth and acc: the files are the restatement of the device
    images; render_view's host outputs are bit-identical before and after"""
    g, r = renderer
    b, Hv, Wv = view_batch()
    host = lambda: {k: v.clone() for k, v in r.render_view(b).items() if torch.is_tensor(v)}          # noqa: E731
    before = host()
    res = r.render_view(b, device_output=True)
    assert res["coarse_color"].is_cuda
    color = res["coarse_color"].cpu().numpy().astype(np.float32)
    p = [str(tmp_path / n) for n in ("c.jpg", "cg.jpg", "d.jpg", "a.jpg", "c2.jpg")]
    size = r.save_views(res, p[0])
    assert open(p[0], "rb").read() == JR.encode(color, 95, "420")[0] and size == os.path.getsize(p[0])
    r.save_views([res], [p[1]], gt=[b], quality=80)
    both = np.concatenate([color, b["img"][0].numpy().astype(np.float32)], 1)
    assert open(p[1], "rb").read() == JR.encode(both, 80, "420")[0]
    for key, path in (("coarse_depth", p[2]), ("coarse_acc", p[3])):
        r.save_views(res, path, key=key)
        img = res[key].cpu().numpy().astype(np.float32).reshape(Hv, Wv)
        assert open(path, "rb").read() == JR.encode(img, 95, "gray")[0], key
    sizes = r.save_views([res, res], [p[0], p[4]], clamp=True, subsampling="444")
    want = JR.encode(np.clip(color, 0, 1), 95, "444")[0]
    assert open(p[0], "rb").read() == open(p[4], "rb").read() == want and sizes == [len(want)] * 2
    with pytest.raises(ValueError):
        r.save_views(res, str(tmp_path / "c.png"))
    after = host()
    assert before.keys() == after.keys()
    for k in before:
        assert torch.equal(before[k].contiguous().view(torch.uint8), after[k].contiguous().view(torch.uint8)), k


def test_rendered_512_frame_against_pillow(J, renderer):
    """a rendered frame brought to 512 x 512 on the device: the encoder's file is the file Pillow writes for the same levels"""
    Image = pytest.importorskip("PIL.Image")
    import io
    g, r = renderer
    b, Hv, Wv = view_batch()
    small = r.render_view(b, device_output=True)["coarse_color"]
    big = torch.nn.functional.interpolate(small.permute(2, 0, 1)[None].float(), size=(512, 512), mode="bilinear")[0].permute(1, 2, 0)
    big = (big + 0.1 * torch.rand(512, 512, 3, device=big.device, generator=torch.Generator(big.device).manual_seed(3))).contiguous()
    got = J.encode(big, quality=95, channels="rgb")[0]
    lv, _ = JR.levels(big.cpu().numpy())
    for q, sub in ((95, 2),):
        buf = io.BytesIO()
        Image.fromarray(lv).save(buf, "JPEG", quality=q, subsampling=sub, optimize=False)
        assert got == buf.getvalue()
