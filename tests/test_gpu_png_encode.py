"""PNG encoding on the device (dsn_png_*, dsn_huff_lengths, dsnerf_amd.png.encode, Renderer.save_views_png / save_test_views) against
the numpy restatement of the rule (tests/png_encode_restate.py, which test_png_encode_host.py holds to zlib, Pillow and the decoder's
restatement): files, lengths, status words and every stage's output are EQUAL, on outputs and workspaces pre-filled with 0xFF
(DSN_POISON_SCRATCH), at sizes on and off the chunk edges, in all three modes and both dtypes."""
import io
import os
import zlib

import numpy as np
import pytest
import torch

import png_encode_restate as R
from helpers import load
from test_png_encode_host import FIB, SIZES, contents, huff_cases

pytestmark = pytest.mark.gpu

MODES = {"grey": 0, "rgb": 1, "replicated": 2}


@pytest.fixture(scope="module")
def L():
    import dsnerf_amd
    return dsnerf_amd._lib


@pytest.fixture(scope="module")
def P():
    import dsnerf_amd
    return dsnerf_amd.png


@pytest.fixture(autouse=True)
def poisoned_outputs(monkeypatch):
    monkeypatch.setenv("DSN_POISON_SCRATCH", "1")          # every output tensor and workspace starts as 0xFF bytes


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def as_mode(stack, mode):
    """frames [F, H, W, 3] -> the encoder's input in this mode and the restatement's keyword arguments"""
    if mode == "rgb":
        return stack, {}
    return np.ascontiguousarray(stack[..., 1]), ({"replicate": True} if mode == "replicated" else {})


def check(out, lengths, status, want, what):
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


def check_stages(L, x, mode, want_stages, rgb, scale, filt, chunk, what):
    """the stages one after the other against the restatement's, and their composition against dsn_png_encode"""
    m = MODES[mode]
    ch = 1 if m == 0 else 3
    H, W = int(x.shape[1]), int(x.shape[2])
    raw, st = L.png_filter(x, m, rgb, scale, filt)
    assert np.array_equal(raw.cpu().numpy(), np.stack([s["raw"] for s in want_stages])), (what, "raw stream")
    adler = L.png_adler(raw)
    assert [int(v) & 0xFFFFFFFF for v in adler.cpu().tolist()] == [s["adler"] for s in want_stages], (what, "adler")
    z, zl, zs = L.png_deflate(raw, ch, 1 + W * ch, chunk)
    check(z, zl, zs, [(s["stream"], 0) for s in want_stages], what + " deflate")
    a = L.png_container(z, zl, adler, W, H, ch, status_in=st, capacity=L.png_encode_max_bytes(W, H, ch, chunk))
    b = L.png_encode(x, m, rgb, scale, filt, chunk)
    n = b[1].cpu().tolist()
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), (what, "composition")
    assert all(torch.equal(a[0][f, :n[f]], b[0][f, :n[f]]) for f in range(len(n))), (what, "composition")
    return b


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_encode_is_the_restatement(L, size, mode):
    W, H = size
    u8 = np.stack(list(contents(H, W, W * 100 + H).values()))
    rng = np.random.default_rng(5)
    wild = (rng.random((H, W, 3)) * 1.5 - 0.25).astype(np.float32)          # values outside [0, 1]
    wild.reshape(-1)[::7] = (np.arange(wild.size)[::7] % 256 + 0.5).astype(np.float32) / np.float32(255.0)      # near ties
    nan = (u8[0] / 255.0).astype(np.float32)
    nan[H // 2, W // 2] = np.nan                                 # (all three channels: the one-channel modes take one of them)
    nan[0, 0] = np.inf
    f32 = np.concatenate([(u8 / 255.0).astype(np.float32), wild[None], nan[None]])
    for stack, rgb in ((u8, False), (f32, True)):
        x, kw = as_mode(stack, mode)
        for chunk in (256, 32768):
            stages = [{} for _ in x]
            want = [R.encode_one(img, channels="rgb" if rgb else "bgr", chunk=chunk, stages=s, **kw) for img, s in zip(x, stages)]
            out, n, st = check_stages(L, dev(x), mode, stages, rgb, 255.0, R.ADAPTIVE, chunk, f"{W}x{H} {mode} c{chunk} {stack.dtype}")
            check(out, n, st, want, f"{W}x{H} {mode} c{chunk} {stack.dtype}")
        if stack is f32:
            assert [w[1] for w in want] == [0, 0, 0, 0, 1]          # the NaN frame alone carries the bit


@pytest.mark.parametrize("chunk", [256, 1024])
def test_raw_sizes_around_the_chunk_edges(L, chunk):
    """one grey row of n - 1 pixels is a raw stream of n bytes: C - 1, C, C + 1 and 2 C + 1"""
    for n in (chunk - 1, chunk, chunk + 1, 2 * chunk + 1):
        rng = np.random.default_rng(n)
        smooth = ((np.arange(n - 1) // 5) * 3 % 256).astype(np.uint8)
        frames = np.stack([smooth, rng.integers(0, 256, n - 1, dtype=np.uint8), np.full(n - 1, 9, np.uint8)])[:, None, :]
        for filt in (R.ADAPTIVE, 0):
            want = [R.encode_one(f, chunk=chunk, filt=filt) for f in frames]
            out, nn, st = L.png_encode(dev(frames), 0, False, 255.0, filt, chunk)
            check(out, nn, st, want, f"n = {n}, chunk {chunk}, filter {filt}")


def test_forced_filters_and_stored_only(L, P):
    img = contents(9, 5, 3)["smooth"]
    two = np.stack([img, img[::-1].copy()])
    for filt in (0, 1, 2, 3, 4, R.ADAPTIVE):
        for mode in sorted(MODES):
            x, kw = as_mode(two, mode)
            want = [R.encode_one(f, filt=filt, chunk=256, **kw) for f in x]
            out, n, st = L.png_encode(dev(x), MODES[mode], False, 255.0, filt, 256)
            check(out, n, st, want, f"filter {filt} {mode}")
    want = [R.encode_one(f, chunk=256, stored_only=True) for f in two]
    out, n, st = L.png_encode(dev(two), 1, False, 255.0, R.ADAPTIVE, 256, stored_only=True)
    check(out, n, st, want, "stored only")
    assert n.cpu().tolist() == [R.encode_max_bytes(5, 9, 3, 256)] * 2
    assert P.encode([dev(f) for f in two], filter="paeth", chunk=256) == [R.encode_one(f, filt=4, chunk=256)[0] for f in two]


# ---- dsn_png_deflate on crafted raw streams ------------------------------------------------------------------------------------------------
def crafted_streams():
    out = {}
    # literal counts follow Fibonacci numbers 1, 2, 3, 5, ... 10946 (20 symbols, 28655 bytes; with the end-of-block symbol's 1 the
    # histogram is 1, 1, 2, 3, 5, ...: a chain 20 deep) and no match is left, so the 15-bit limit is hit.  A random shuffle cannot do it
    # (the two most frequent symbols are 62 % of the bytes: three equal bytes in a row are certain), so the sorted bytes are read with a
    # fixed stride of 0.45 n, coprime to n: neighbours lie 0.45 n apart in the sorted array and the largest block is 0.38 n long, so no
    # two neighbours are equal
    base = np.concatenate([np.full(FIB[k + 1], 40 + k, np.uint8) for k in range(20)])
    raw = base[np.arange(len(base)) * 12894 % len(base)]
    plans = []
    R.deflate(raw, 1, 30000, 32768, plans=plans)
    assert sorted(np.bincount(raw)[40:60].tolist()) == FIB[1:21] and all(len(t) == 1 for t in plans[0]["tokens"])
    assert max(plans[0]["ll_lens"]) == 15 and max(R.huff_lengths(plans[0]["ll_hist"], 15, mutant_no_limit=True)) == 20
    assert plans[0]["btype"] == 2
    out["fibonacci literals"] = (raw, 1, 30000, 32768)
    # a run that crosses a 64-position group and a chunk edge
    run = np.random.default_rng(1).integers(0, 256, 700, dtype=np.uint8)
    run[30:200] = 7
    run[230:300] = 9
    out["run across groups and a chunk edge"] = (run, 1, 701, 256)
    # a chunk with no match at all, and one with exactly one distance symbol
    out["no match"] = ((np.arange(256) * 7 % 16).astype(np.uint8), 1, 300, 256)          # 16 symbols, neighbours differ
    one = (np.arange(300) * 7 % 16).astype(np.uint8)
    one[100:110] = one[99]
    out["one distance symbol"] = (one, 1, 301, 512)
    wide = np.random.default_rng(2).integers(0, 16, 3000, dtype=np.uint8)
    wide[1500:1520] = wide[1500 - 1000:1520 - 1000]
    out["row distance 1000"] = (wide, 4, 1000, 4096)
    return out


@pytest.mark.parametrize("name", ["fibonacci literals", "run across groups and a chunk edge", "no match", "one distance symbol", "row distance 1000"])
def test_deflate_of_crafted_streams(L, name):
    raw, bpp, stride, chunk = crafted_streams()[name]
    plans = []
    want = R.deflate(raw, bpp, stride, chunk, plans=plans)
    assert zlib.decompress(want, -15) == raw.tobytes()
    if name == "no match":
        assert all(len(t) == 1 for t in plans[0]["tokens"])
    if name == "one distance symbol":
        assert sum(1 for n in plans[0]["d_hist"] if n) == 1 and sum(plans[0]["d_hist"]) == 1
    if name == "row distance 1000":
        assert any(len(t) == 2 and t[1] == 1000 for t in plans[0]["tokens"]) and any(len(t) == 2 and t[1] < 5 for t in plans[0]["tokens"])
    if name != "run across groups and a chunk edge":
        assert plans[0]["btype"] != 0
    out, n, st = L.png_deflate(dev(np.stack([raw, raw[::-1].copy()])), bpp, stride, chunk)
    check(out, n, st, [(want, 0), (R.deflate(raw[::-1].copy(), bpp, stride, chunk), 0)], name)
    short = L.png_deflate(dev(raw[None]), bpp, stride, chunk, capacity=len(want) - 1)
    assert short[1].cpu().tolist() == [len(want)] and short[2].cpu().tolist() == [L.PNGE_OVERFLOW]
    assert short[0].cpu().numpy()[0].tobytes() == want[:-1]


def test_huff_lengths(L):
    for counts, limit in huff_cases():
        if len(counts) > (1 << limit):
            continue
        got = L.huff_lengths(dev(np.array([counts, counts[::-1]], np.int32)), limit).cpu().numpy()
        assert got[0].tolist() == R.huff_lengths(counts, limit), (len(counts), limit)
        assert got[1].tolist() == R.huff_lengths(counts[::-1], limit), (len(counts), limit, "reversed")


# ---- batches and capacity ----------------------------------------------------------------------------------------------------------------------
def test_batches_equal_single_calls(L):
    """F = 1, 2, 3, 5 and a permuted batch give each frame the bytes of its own call; frames of very different lengths side by side"""
    c = contents(37, 53, 21)
    frames = np.stack([c["noise"], c["constant"], c["smooth"], c["noise"][::-1].copy(), c["constant"]])
    single = []
    for f in range(5):
        out, n, st = L.png_encode(dev(frames[f:f + 1]), 1, chunk=1024)
        single.append(out[0, :int(n[0])].cpu().numpy().tobytes())
    assert max(len(s) for s in single) > 4 * min(len(s) for s in single)
    assert single == [R.encode_one(f, chunk=1024)[0] for f in frames]
    for order in ([0], [0, 1], [0, 1, 2], [0, 1, 2, 3, 4], [4, 2, 0, 3, 1]):
        out, n, st = L.png_encode(dev(frames[order]), 1, chunk=1024)
        check(out, n, st, [(single[k], 0) for k in order], f"batch {order}")


def test_capacity_one_byte_short(L):
    """a frame that needs one byte more than the capacity: OVERFLOW for it alone, the needed length reported, nothing written at or
    past the capacity (its row's last byte is the neighbour's first), the guard behind the buffer untouched"""
    c = contents(40, 48, 31)
    frames = np.stack([c["constant"], c["noise"], c["constant"]])
    want = [R.encode_one(f, chunk=1024)[0] for f in frames]
    cap = len(want[1]) - 1
    assert len(want[0]) < cap
    big = torch.full((3 * cap + 256,), 0xAB, dtype=torch.uint8, device="cuda")
    out, n, st = L.png_encode(dev(frames), 1, chunk=1024, out=big[:3 * cap].view(3, cap))
    assert n.cpu().tolist() == [len(w) for w in want]
    assert st.cpu().tolist() == [0, L.PNGE_OVERFLOW, 0]
    got = big.cpu().numpy()
    assert (got[3 * cap:] == 0xAB).all()
    for f in (0, 2):
        row = got[f * cap:(f + 1) * cap]
        assert row[:len(want[f])].tobytes() == want[f] and (row[len(want[f]):] == 0xAB).all()
    assert got[cap:2 * cap].tobytes() == want[1][:cap]          # what fits is the file's beginning


def test_repeated_and_unpoisoned_calls_have_the_same_bytes(L, monkeypatch):
    x = dev(np.stack(list(contents(63, 65, 41).values())))
    a = L.png_encode(x, 1)
    b = L.png_encode(x, 1)
    monkeypatch.delenv("DSN_POISON_SCRATCH")
    c = L.png_encode(x, 1)
    n = a[1].cpu().tolist()
    for other in (b, c):
        assert torch.equal(a[1], other[1]) and torch.equal(a[2], other[2])
        assert all(torch.equal(a[0][f, :n[f]], other[0][f, :n[f]]) for f in range(3))


def test_constant_image_and_bounds(L, P):
    img = np.empty((256, 256, 3), np.uint8)
    img[...] = np.array([77, 130, 200])
    data = P.encode(img)[0]
    assert data == R.encode_one(img)[0] and len(data) < 0.03 * img.size
    assert L.png_encode_max_bytes(256, 256, 3) == R.encode_max_bytes(256, 256, 3)


# ---- round trips and the module's surface --------------------------------------------------------------------------------------------------------
def test_module_surface_and_round_trip(P, tmp_path):
    """lists, [H, W, 1], non-contiguous and host inputs, float64; decode(encode(x)) on the device; imwrite's params and extension check"""
    c = np.stack(list(contents(37, 53, 51).values()))
    want = [R.encode_one(f)[0] for f in c]
    assert P.encode([dev(f) for f in c]) == want
    assert P.encode(c) == want                                              # a host stack is uploaded
    wide = dev(np.concatenate([c, c], 2))
    assert P.encode(wide[:, :, :53]) == want                                # non-contiguous rows
    assert P.encode((c / 255.0).astype(np.float64)) == want                 # float64 is cast to float32
    grey = c[0, :, :, :1]
    assert P.encode(grey) == P.encode(grey[..., 0]) == [R.encode_one(grey[..., 0])[0]]
    assert P.encode(grey, replicate=True) == [R.encode_one(grey[..., 0], replicate=True)[0]]
    assert P.encode(c[0], channels="rgb", filter="sub", chunk=256) == [R.encode_one(c[0], channels="rgb", filt=1, chunk=256)[0]]
    buf, n, st = P.encode_device(dev(c))
    assert buf.is_cuda and n.is_cuda and st.is_cuda and n.cpu().tolist() == [len(w) for w in want]
    back = P.decode(P.encode(dev(c)))
    assert back.is_cuda and torch.equal(back, dev(c))
    assert torch.equal(P.decode(P.encode(dev(c[..., 0])), channels="native")[..., 0], dev(c[..., 0]))
    p = tmp_path / "a.png"
    lv = (np.random.default_rng(1).random((16, 17, 3)) * 300 - 20).astype(np.float32)          # cv2.imwrite(path, img * 255): levels as floats
    assert P.imwrite(str(p), torch.from_numpy(lv)) is True
    assert p.read_bytes() == R.encode_one(lv, scale=1.0)[0]
    P.imwrite(str(p), c[0], [P.IMWRITE_PNG_COMPRESSION, 0])
    assert p.read_bytes() == R.encode_one(c[0], stored_only=True)[0]
    P.imwrite(str(p), c[0], [P.IMWRITE_PNG_COMPRESSION, 3])
    assert p.read_bytes() == want[0]
    with pytest.raises(ValueError, match="jpeg.imwrite"):
        P.imwrite(str(tmp_path / "a.jpg"), c[0])
    with pytest.raises(ValueError):
        P.imwrite(str(p), c[0], [1, 90])
    with pytest.raises(ValueError):
        P.encode([c[0], c[0][:8]])
    with pytest.raises(ValueError):
        P.encode(c[0], replicate=True)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------
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


def levels_of(data):
    Image = pytest.importorskip("PIL.Image")
    return np.asarray(Image.open(io.BytesIO(data)))


@pytest.mark.parametrize("poison", [True, False])
def test_save_views_end_to_end(renderer, tmp_path, monkeypatch, poison):
    """render_view(device_output=True) -> save_views_png and save_test_views: the files are the restatement of the device images, zlib
    and Pillow return their levels, the side-by-side file is the encode of the joined image; render_view's host outputs are
    bit-identical before and after"""
    if not poison:
        monkeypatch.delenv("DSN_POISON_SCRATCH")
    g, r = renderer
    b, Hv, Wv = view_batch()
    host = lambda: {k: v.clone() for k, v in r.render_view(b).items() if torch.is_tensor(v)}          # noqa: E731
    before = host()
    res = r.render_view(b, device_output=True)
    color = res["coarse_color"].cpu().numpy().astype(np.float32)
    gt = b["img"][0].numpy().astype(np.float32)
    p = [str(tmp_path / n) for n in ("c.png", "cg.png", "d.png", "a.png")]
    size = r.save_views_png(res, p[0])
    data = open(p[0], "rb").read()
    assert data == R.encode_one(color)[0] and size == len(data)
    lv = R.levels(color)[0]
    assert np.array_equal(levels_of(data), lv[:, :, ::-1])
    assert zlib.decompress(R.idat_payload(data))[0] <= 4
    r.save_views_png([res], [p[1]], gt=[b], clamp=True)
    both = np.concatenate([np.clip(color, 0, 1), gt], 1)
    assert open(p[1], "rb").read() == R.encode_one(both)[0]
    for key, path in (("coarse_depth", p[2]), ("coarse_acc", p[3])):
        r.save_views_png(res, path, key=key, replicate=True)
        img = res[key].cpu().numpy().astype(np.float32).reshape(Hv, Wv)
        assert open(path, "rb").read() == R.encode_one(img, replicate=True)[0], key
        assert levels_of(open(path, "rb").read()).shape == (Hv, Wv, 3)
    with pytest.raises(ValueError):
        r.save_views_png(res, str(tmp_path / "c.jpg"))
    dirs = {k: tmp_path / k for k in r.TEST_VIEW_KINDS}
    for d in dirs.values():
        d.mkdir()
    sizes = r.save_test_views([res, res], [b, b], dirs, ["frame0000_view0000", "frame0001_view0000"])
    depth = res["coarse_depth"].cpu().numpy().astype(np.float32).reshape(Hv, Wv)
    acc = res["coarse_acc"].cpu().numpy().astype(np.float32).reshape(Hv, Wv)
    want = {"img": R.encode_one(both)[0], "rendering": R.encode_one(np.clip(color, 0, 1))[0], "gt": R.encode_one(gt)[0],
            "depth": R.encode_one(depth, replicate=True)[0], "acc": R.encode_one(acc, replicate=True)[0]}
    assert sorted(sizes) == sorted(want)
    for kind, data in want.items():
        files = sorted(os.listdir(dirs[kind]))
        assert files == ["frame0000_view0000.png", "frame0001_view0000.png"], kind
        for n, f in zip(sizes[kind], files):
            assert (dirs[kind] / f).read_bytes() == data and n == len(data), kind
    assert levels_of(want["img"]).shape == (Hv, 2 * Wv, 3)
    after = host()
    assert before.keys() == after.keys()
    for k in before:
        assert torch.equal(before[k].contiguous().view(torch.uint8), after[k].contiguous().view(torch.uint8)), k
